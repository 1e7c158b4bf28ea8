"""What tests/scan_edges.py claims, shown without a GPU: the plain count equals the oracle's all-pairs scores on every case (so the oracle vouches
for the judge of tests/test_scan_edges_gpu.py), no query is dropped by the preparation, and -- by the model of host_qtables.inc's classification,
from the prepared queries alone -- every case reaches the edge of the stream, the tile range or the counter half it is built for."""
import numpy as np
import pytest

import scan_edges as SE

MODES = [(k, a) for k, c in SE.CASES.items() for a in c.modes]
by_mode = pytest.mark.parametrize("key,acgt", MODES, ids=["%s-%s" % (k, "acgt" if a else "iupac") for k, a in MODES])


def model(key, nw=8):
    return SE.model(key, SE.CASES[key].modes[0], nw)


def records(key, st=0, nw=8):
    return {r.g: r for r in model(key, nw).records[st]}


@by_mode
def test_plain_count_equals_the_oracle(key, acgt):
    """default: first == S[0], second == S[3];  --acgt: first == S[1] - S[0], second == S[1] (Query.allpairs, untruncated)"""
    c, q = SE.CASES[key], SE.query(key, acgt)
    assert q.ntax == c.nq, "the preparation dropped a query"
    first, second, _valid, _pre = SE.gold(key, acgt)
    S = q.allpairs(list(c.refs))                                           # [n_ref, ntax, 6]
    if acgt:
        assert np.array_equal(first.T, S[:, :, 1] - S[:, :, 0]) and np.array_equal(second.T, S[:, :, 1])
    else:
        assert np.array_equal(first.T, S[:, :, 0]) and np.array_equal(second.T, S[:, :, 3])
    assert int(second.max()) < 65536 and int(first.min()) >= 0


def test_plain_count_by_hand():
    q, r = [b"ACGTNR-AC"], [b"ACGAARCNT", b"NNNNNNNNN"]
    f, s = SE.plain_count(q, r, 0, False)
    assert f.tolist() == [[3, 0]] and s.tolist() == [[6, 0]]              # valid pairs: A C G T/A R/R C/T
    f, s = SE.plain_count(q, r, 0, True)
    assert f.tolist() == [[2, 0]] and s.tolist() == [[5, 0]]
    f, s = SE.plain_count(q, r, 3, False)
    assert f.tolist() == [[0, 0]] and s.tolist() == [[2, 0]]
    assert SE.plain_valid_sites(r).tolist() == [8, 0]
    b = SE.plain_bounds(np.array([[5, 1, 7]]), np.array([[9, 9, 8]]), False, 1, 2)
    assert b.tolist() == [[[1, 7]]]


def test_every_group_has_its_cases_and_every_instantiation_a_run():
    assert {c.group for c in SE.CASES.values()} == set("SWPTCK")
    runs = SE.runs()
    assert {(a, v) for _k, a, v, _c in runs if v is not None} == {(a, v) for a in (False, True) for v in SE.SCAN3}
    scan2 = {(SE.qt2(SE.CASES[k].nq), a, c) for k, a, v, c in runs if v is None}
    assert scan2 == {(qt, a, c) for qt in (1, 2, 4, 8, 16) for a in (False, True) for c in (False, True)}
    for c in SE.CASES.values():
        assert c.aim and 3 <= c.nq <= 130 or c.group == "K"
        assert max(n for n, _r in c.scans) <= 640                          # max_pool of the contexts


# ------------------------------------------------------------------------------------------------------------------ S
def test_s_reaches_every_list_shape():
    want, rec = SE.CASES["S"].meta["want"], records("S")
    m = model("S")
    assert m.n_st == 2 and m.variant == 2 and m.NP4 == 1 and m.NR4 == 0
    for g, k in want["full"]:                                              # S1: n_full4 = 1, 1, 1, 2, 2, 16; padded except at 4, 8 and 64
        assert len(rec[g].full) == k and not rec[g].gen and not any(rec[g].words), g        # S5: a record with only a full list
    assert sorted(len(rec[g].full) for g, _k in want["full"]) == [1, 3, 4, 5, 8, 64]
    for g, k in want["gen"]:                                               # S2: the `k + 1 < n_gen` arm is skipped at 1 and 3, taken at 2 and 63
        assert len(rec[g].gen) == k and not rec[g].full, g
    for g, counts in want["words"]:                                        # S3 (and S5: records with only word items)
        assert tuple(len(w) for w in rec[g].words) == counts and not rec[g].gen and not rec[g].full and not rec[g].any_run, g
    for g, word, fm in want["runs"]:                                       # S4
        items = [(j, f) for j in range(4) for _q, f in rec[g].words[j]]
        assert (word, fm) in items and not rec[g].gen, (g, items)
        assert rec[g].any_run == (fm != 0)
    assert sorted(fm for _g, _w, fm in want["runs"]) == [0, 0xFF00, 0xFF00, 0xFFFF00, 0xFFFF00, 0xFFFFFF00]
    mixed = [g for g, _w, fm in want["runs"] if fm and any(f == 0 for j in range(4) for _q, f in rec[g].words[j])]
    assert mixed                                                           # `h.v[0] & 1u` set and an item with `cur.v[3] == 0` in the same record
    r = rec[want["all3"]]
    assert r.full and r.gen and any(r.words)
    tail = rec[m.W4 - 1]                                                   # the alignment ends inside the last group: a run item for every query
    assert sum(len(w) for w in tail.words) == 64 and tail.any_run
    # dirty characters that are valid but not ACGT (~qV and ~qI & constMask differ), and dirty polymorphic columns (nI clear, nV set)
    assert (m.nI & ~m.nV).any() and (m.nV[:, :m.nchar] & ~m.nI[:, :m.nchar] & m.dense[None, :m.nchar]).any()


def test_s_trim_makes_whole_groups_all_n():
    m, rec = model("S-trim"), records("S-trim")
    assert len(rec[0].full) == 64 and len(rec[m.W4 - 1].full) == 64        # groups 0 and 23 lie outside [130, 2870)
    assert not rec[0].gen and not any(rec[0].words)
    assert any(rec[1].words) or rec[1].gen                                 # the trim ends inside group 1


# ------------------------------------------------------------------------------------------------------------------ W
def test_w1_waves_without_records_and_with_an_odd_number():
    m = model("W1", 8)
    assert len(m.records[0]) == 3
    sh = m.record_shares(0)
    assert sum(sh) == 3 and 0 in sh and any(s % 2 for s in sh)
    assert sum(model("W1", 4).record_shares(0)) == 3


def test_w2_a_clean_super_tile():
    m = model("W2")
    assert m.records[0] and not m.records[1] and m.NR4 == 0
    assert m.record_shares(1) == [0] * 8


def test_w3_super_tiles():
    for n, last in ((33, 33), (64, 64), (65, 1), (130, 2)):
        m = model("W3-%d" % n)
        assert m.nq == n and m.n_st == 2 * ((n + 127) // 128)
        st = (n - 1) // 64
        assert {q for r in m.records[st] for q in r.full + r.gen + [x for w in r.words for x, _f in w]} <= set(range(last))
        assert m.records[st]
    assert SE.written_rows(130, 2, (64, 128)) == (64, 128) and SE.CASES["W4"].active == (64, 128)


# ------------------------------------------------------------------------------------------------------------------ P
@pytest.mark.parametrize("key", [k for k, c in SE.CASES.items() if c.group == "P"])
def test_p_column_counts(key):
    m, meta = model(key), SE.CASES[key].meta
    assert (m.NP, m.NR) == (meta["NP"], meta["NR"]) and m.variant == 2
    assert m.NP4 == (m.NP + 127) // 128 and m.NR4 == (m.NR + 127) // 128


def test_p_shapes():
    assert model("P1").NP4 == 0 and [model("P2-%d" % n).NP4 for n in (1, 128, 129)] == [1, 1, 2]
    assert model("P3-rare").NP4 == 0 and model("P3-rare").NR4 == 1 and model("P3-dense").NR4 == 0 and model("P3-dense").NP4 == 1
    m = model("P456")
    assert m.NP4 == 1 and m.NR4 == 3                                       # the second and third rare record sit behind the dense group
    counts = [{r.r4: tuple(len(w) for w in r.words) for r in m.rare_records[st]} for st in range(2)]
    assert counts[0] == {0: (1, 0, 0, 0), 1: (0, 0, 0, 1), 2: (2, 3, 1, 4)}, counts
    assert counts[1] == {0: (0, 1, 1, 1), 1: (1, 1, 1, 0)}, counts
    # P6: a query that is N at a rare column has no rare item for it, and is dirty there through the normal items
    col = int(np.nonzero(m.rare)[0][300])
    q = [i for i in range(m.nq) if not m.qI[i, col]]
    assert len(q) == 1 and m.nV[q[0], col] and m.nI[q[0], col]
    assert sum(bool(s >> (300 & 31) & 1) for _q, s in m.rare_records[0][2].words[300 // 32 % 4]) == 1


# ------------------------------------------------------------------------------------------------------------------ T
def test_t_tiles_and_grid():
    assert [(n + 63) // 64 for n, _r in SE.CASES["T1"].scans] == [1, 2, 3, 5]
    (n, ranges), = SE.CASES["T2"].scans
    assert n % 64 and ranges == [(0, 191), (37, 1), (37, 27), (63, 2), (64, 64), (100, n - 100)]
    c = SE.CASES["T3"]
    tiles, n_st = (len(c.refs) + 63) // 64, (c.nq + 63) // 64
    assert tiles == 9 and n_st == 2 and n_st * ((tiles + 7) // 8) * 8 == 32 > n_st * tiles       # scan_grid_size: slots without a tile group


# ------------------------------------------------------------------------------------------------------------------ C
def test_c1_low_half_close_to_two_to_the_16():
    """the low counter half of (query, reference) is SCAN3_BIAS + 128 NP4 + te - first, te = the reference's matches with the constant bases"""
    c, m = SE.CASES["C1"], model("C1")
    assert m.nchar == SE.WIDE_ABOVE and m.variant == 2 and m.NP4 == 1
    first, second, _v, _p = SE.gold("C1", False)
    R = SE.as_array(c.refs)
    base = SE.as_array(SE.query("C1", False).seqs)
    cons = np.where(m.cmask[:m.nchar], [max((b for b in col if b in b"ACGT"), default=0) for col in base.T], 0)
    te = (R == cons[None, :]).sum(axis=1)
    low = SE.SCAN3_BIAS + 128 * m.NP4 + te[None, :] - first
    assert 65536 - 64 <= int(low.max()) < 65536, int(low.max())            # built input: 65 479, i.e. 57 below 2^16
    assert int(second[0].max()) == 32                                      # the query that is N outside one word (first after the reordering)


def test_c2_c3_on_both_sides_of_the_bias():
    m2, m3 = model("C2"), model("C3")
    assert (m2.NP4, m2.NR4, m2.variant) == (126, 0, 2) and (m3.NP4, m3.NR4, m3.variant) == (127, 0, 0)
    first, _s, _v, _p = SE.gold("C2", True)
    dense = first[:, 1].min()                                              # reference 1 mismatches every query on every polymorphic column
    assert dense >= 126 * 128 and SE.SCAN3_BIAS - 126 * 128 == 256


# ------------------------------------------------------------------------------------------------------------------ K
def test_k_query_tiles():
    assert [SE.qt2(n) for n in (1, 2, 3, 5, 8, 9, 17, 32)] == [1, 2, 4, 8, 8, 16, 16, 16]
    for n in (1, 2, 3, 5, 8, 9, 17, 32):
        c = SE.CASES["K-%d" % n]
        assert c.nq == n and c.cons == (True, False)
        for acgt in c.modes:
            assert len(SE.query(c.key, acgt).idx_c) > 0                    # CONS runs as prepared; the other run moves idx_c into idx_m
    assert [SE.written_rows(n, 0)[1] for n in (3, 5, 9, 17)] == [4, 8, 16, 32]
