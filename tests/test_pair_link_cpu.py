"""Single-linkage clusters without a GPU: the constructed cases have the structure their tests on the GPU rely on (asserted from the
oracle's counters), the restatement gives the same clusters from the oracle's counters and from the plane formulas, and what
`uvaiadist --clusters` refuses before the engine opens."""
import os
import subprocess

import numpy as np
import pytest

import pair_dist as D
import pair_link as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIADIST = os.path.join(ROOT, "bin", "uvaiadist")


def test_chains_have_their_structure():
    seqs, family, member = K.chains()
    c = K.counts("chains260x513")
    n = len(seqs)
    assert n == 260 and all(len(s) == 513 for s in seqs)
    assert (c[..., 4] == 513).all()                                   # ACGT everywhere: the floor never bites
    d = D.snp(c)
    assert np.array_equal(d, D.uvaia(c))
    family, member = np.array(family), np.array(member)
    same = family[:, None] == family[None, :]
    assert np.array_equal(d[same], np.abs(member[:, None] - member[None, :])[same])      # a chain: |k - k'| inside a family
    assert d[~same].min() >= 6                                        # three signature substitutions on either side
    assert sorted(np.bincount(family).tolist()) == sorted(K.CHAIN_FAMILIES)
    for f, members in enumerate(K.CHAIN_FAMILIES):
        if members > 60:
            assert set((np.flatnonzero(family == f) // 64).tolist()) == {0, 1, 2, 3, 4}, f       # every large family spans all five tiles
    head, tail = (int(np.flatnonzero((family == 6) & (member == k))[0]) for k in (0, 64))
    assert d[head, tail] == 64
    for metric in ("snp", "uvaia"):
        labels, links = K.restate(c, metric, 1)
        assert len(set(labels.tolist())) == 8 and links == sum(m - 1 for m in K.CHAIN_FAMILIES)
        assert sorted(np.bincount(labels)[np.unique(labels)].tolist()) == sorted(K.CHAIN_FAMILIES)
        assert all(labels[i] == np.flatnonzero(family == family[i])[0] for i in range(n))
        assert labels[head] == labels[tail]
        labels, links = K.restate(c, metric, 0)
        assert np.array_equal(labels, np.arange(n)) and links == 0


def test_dense_rows_are_one_cluster():
    c = K.counts("dense130")
    for metric in ("snp", "uvaia"):
        labels, links = K.restate(c, metric, 0)
        assert not labels.any() and links == 130 * 129 // 2


def test_special_rows_and_the_floor():
    """under snp an all-N (or all-gap) row is at distance 0 from every row: with no floor it joins everything, which is the definition"""
    c = K.counts("special129")
    assert not c[0].any() and not c[1].any()
    assert D.snp(c)[3, 5] > 2 and D.snp(c)[3, 4] == 0
    labels, links = K.restate(c, "snp", 0, min_compared=0)
    assert not labels.any() and links >= 11
    labels, _links = K.restate(c, "snp", 0, min_compared=1)
    assert labels.tolist() == [0, 1, 2, 3, 3, 5]                      # the partial-codes row has no ACGT site either


@pytest.mark.parametrize("metric", ["snp", "uvaia"])
@pytest.mark.parametrize("max_dist", [0, 1, 2])
def test_synth130_is_neither_one_cluster_nor_all_singletons(max_dist, metric):
    c = K.counts("synth130")
    for floor in (0, K.SYNTH_FLOOR):
        labels, links = K.restate(c, metric, max_dist, floor)
        assert 1 < len(set(labels.tolist())) < 130 and 0 < links < 8385, (floor, links)
        assert (labels <= np.arange(130)).all() and (labels[labels] == labels).all()
    if metric == "snp":
        assert K.restate(c, metric, max_dist)[1] == {0: 1561, 1: 4441, 2: 6777}[max_dist]
    assert K.restate(c, metric, max_dist, K.SYNTH_FLOOR)[1] < K.restate(c, metric, max_dist)[1]       # the floor takes links away


@pytest.mark.parametrize("name", ["chains260x513", "special129", "synth130", "awkward9x129"])
def test_oracle_counters_and_plane_counters_give_the_same_clusters(name):
    seqs, nchar = K.case(name)
    for trim in (0, 33):
        a, b = D.oracle_counts_of(seqs, trim) if trim else K.counts(name), D.plane_counts_of(seqs, nchar, trim)
        for metric in ("snp", "uvaia"):
            for max_dist, floor in ((0, 0), (1, 0), (2, 1), (1, 90), (1, K.SYNTH_FLOOR - 2 * trim)):
                la, na = K.restate(a, metric, max_dist, floor)
                lb, nb = K.restate(b, metric, max_dist, floor)
                assert np.array_equal(la, lb) and na == nb, (trim, metric, max_dist, floor)


def test_a_rectangle_links_only_its_own_pairs():
    c = K.counts("chains260x513")
    whole, n_whole = K.restate(c, "snp", 1)
    part, n_part = K.restate(c, "snp", 1, rows=(31, 34))
    rest = [K.restate(c, "snp", 1, rows=r)[1] for r in ((0, 31), (65, 195))]
    assert 0 < n_part < n_whole and n_part + sum(rest) == n_whole
    assert len(set(part.tolist())) == 260 - n_part                   # a forest: every link of a chain joins two components
    assert (part >= whole).all()


def test_the_text_numbers_clusters_by_first_member():
    labels = np.array([0, 1, 0, 3, 1, 1], dtype=np.uint32)
    names = list("abcdef")
    assert K.clusters_text(names, labels) == b"a\t1\t2\nb\t2\t3\nc\t1\t2\nd\t3\t1\ne\t2\t3\nf\t2\t3\n"
    assert K.clusters_text(names, labels, sep=",", min_size=3) == b"b,2,3\ne,2,3\nf,2,3\n"


def test_the_matrix_product_restatement_of_snp_links():
    seqs, _nchar = K.case("synth130")
    rows = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(130, -1)
    for trim in (0, 33):
        c = D.oracle_counts_of(seqs, trim) if trim else K.counts("synth130")
        want = np.argwhere(K.linked(c, "snp", 1) & (np.arange(130)[:, None] < np.arange(130)[None, :]))
        got = K.snp_links_of_bytes(rows, trim, 1, block=64)
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist()))


# ---- uvaiadist: what is refused before the engine opens, each by its own message
@pytest.mark.parametrize("args, message", [
    (("--clusters", "--stdout", "x.fa"), b"--clusters needs -d"),
    (("-d", "1", "--clusters", "--long", "--stdout", "x.fa"), b"--clusters does not go with --long"),
    (("-d", "1", "--clusters", "--counts", "--stdout", "x.fa"), b"--clusters does not go with --counts"),
    (("-d", "1", "--clusters", "--dense", "--stdout", "x.fa"), b"--clusters does not go with --dense"),
    (("-d", "1", "--min-compared", "5", "--stdout", "x.fa"), b"--min-compared needs --clusters"),
    (("-d", "1", "--min-size", "2", "--stdout", "x.fa"), b"--min-size needs --clusters"),
    (("-d", "1", "--clusters", "--min-compared", "-1", "--stdout", "x.fa"), b"--min-compared takes a number of 0 or more"),
    (("-d", "1", "--clusters", "--min-size", "-2", "--stdout", "x.fa"), b"--min-size takes a number of 0 or more"),
    (("-d", "-1", "--clusters", "--stdout", "x.fa"), b"-d takes a distance of 0 or more"),
])
def test_cluster_refusals_need_no_gpu(args, message):
    r = subprocess.run([UVAIADIST, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert not r.stdout                                               # its own message, not the usage text
