"""The inputs of tests/cluster_edges.py do what they are built for, shown on the restatements of the reference (no GPU): each group's
conditions below are what makes a pass of tests/test_cluster_edges_gpu.py mean something, and they fail if an edit of a builder
empties a case."""
import numpy as np
import pytest

import cluster_edges as E
import cluster_lib as CL
import packed_lib as P


# ------------------------------------------------------------------------------------- A: more medoids than the LDS part of the list
def test_group_a_crosses_the_lds_part_of_the_medoid_list():
    ref, seqs, queues, named = E.group_a()
    assert E.A_PUSHES[-1] < len(seqs) and len(ref) == E.A_NCHAR
    clusters, scores = CL.rs_cluster(ref, seqs, queues, 0, 0, 1, 1)
    slot = {o: k for k, o in enumerate(sorted(m for m, _ in clusters))}        # one queue: medoids take their slots in push order
    assert len(slot) >= E.LDS_ST + 128
    # the last push starts with more than LDS_ST medoids in the queue
    assert sum(1 for o in slot if o < E.A_PUSHES[-1]) > E.LDS_ST
    stored1 = sorted(slot[m] for (m, _), s in zip(clusters, scores.tolist()) if s[0] == 1)
    low, high = [s for s in stored1 if s < E.LDS_ST], [s for s in stored1 if s >= E.LDS_ST]
    assert low and high
    assert high[0] - low[-1] < 4                                               # one ballot window holds both sides of the boundary
    assert E.LDS_ST - 1 in stored1 and E.LDS_ST in stored1
    assert [slot[o] for o in named["extras"]] == [s for s, _, _ in E.A_EXTRAS]
    assert set(slot[o] for o in named["extras"]) < set(stored1)
    members = {m: mem for m, mem in clusters}
    # a join to a medoid read from global memory, as ring hit and as a later candidate
    assert members[named["plain_global"]] == [named["dup_plain"]] and slot[named["plain_global"]] > E.LDS_ST
    far = named["extras"][6]
    assert members[far] == [named["dup_extra"]] and slot[far] > E.LDS_ST
    assert sum(len(m) for m in members.values()) == 2
    # a founder with stored 1 beyond the boundary, after candidates on both sides of it
    assert slot[named["late_founder"]] > E.LDS_ST and slot[named["late_founder"]] in stored1


# ------------------------------------------------------------------------------------------------------------- B: window edges
def test_group_b_keeps_every_shape():
    shapes = [(n, t, p) for n in E.B_NCHARS for t, p in E.group_b_shapes(n)]
    assert 100 <= len(shapes) <= 150
    for n in E.B_NCHARS:
        mine = [(t, p) for m, t, p in shapes if m == n]
        assert sorted({t for t, _ in mine}) == sorted(t for t in {0, 1, 15, 16, 17, int(n / 2.1)} if 2 * t < n)
        for p in (0, 2, 17):
            assert any(q == p for _, q in mine) == (p < n)
    assert {t % 16 for _, t, _ in shapes} >= {0, 1, 15, 7, 8, 12, 14}           # 0, 1, 15, 16, 17 and nchar / 2.1 of 15, 17, 1 000, 4 097, ...


def test_group_b_edges_decide():
    n_cases = both = shift_decides = 0
    merge_differs = set()
    trims = set()
    for nchar in E.B_NCHARS:
        for trim, p0, dist, ref, rows in E.group_b_cases(nchar):
            n_cases += 1
            trims.add(trim)
            one = CL.rs_cluster(ref, rows, [0] * len(rows), dist, trim, 1, 1)
            two = CL.rs_cluster(ref, rows, E.alternate(len(rows)), dist, trim, 1, 2)
            flat = CL.rs_cluster(ref, rows, [0] * len(rows), dist, trim, 0, 1)
            joined = sum(len(m) for _, m in one[0])
            both += 0 < joined and len(one[0]) > 1                             # some twins join, others found
            shift_decides += one[0] != flat[0]
            if two[0] != one[0]:
                merge_differs.add(trim)
            if len(rows) * nchar < 40000:
                for q, nq, want in (([0] * len(rows), 1, one), (E.alternate(len(rows)), 2, two)):
                    py = CL.py_cluster(ref, rows, q, dist, trim, 1, nq)
                    assert py[0] == want[0] and py[1].tolist() == want[1].tolist(), (nchar, trim, p0, dist, nq)
    assert both * 3 >= n_cases, (both, n_cases)
    assert shift_decides * 3 >= n_cases, (shift_decides, n_cases)
    assert merge_differs >= trims - {0}, sorted(trims - merge_differs)


# ------------------------------------------------------------------------------------------------- C: positions, counts, bytes
@pytest.mark.parametrize("trim", E.C_TRIMS)
@pytest.mark.parametrize("n_score", E.C_N_SCORES)
def test_group_c_positions(trim, n_score):
    ref, rows, want = E.group_c(trim, n_score)
    assert len(set(rows)) == len(rows)
    clusters, scores = CL.rs_cluster(ref, rows, [0] * len(rows), 0, trim, n_score, 1)
    E.check_group_c(clusters, scores, want, n_score)
    margins = sum(1 for w in want[1:] if w[0] == 0)
    assert margins >= 5 if trim else margins == 0
    assert len(clusters) == len(rows) - margins                                # the margin rows join the row without differences
    assert dict(clusters)[0] == [k for k in range(1, len(rows)) if want[k][0] == 0]
    counts = {w[0] for w in want}
    assert counts >= {0, 1, 2, 16, 70, 90} and {k for k in (n_score - 1, n_score, n_score + 1) if k > 0} <= counts
    if n_score == 70:
        assert any(w[0] == 70 and w[-1] - w[1] > 4 * 1024 for w in want)       # total < n_score over several chunks


def test_group_bytes_upper_casing_decides():
    ref, rows = E.group_bytes()
    assert all(len(r) == E.BYTES_NCHAR for r in rows + [ref])
    for j in range(4):                                                         # every byte at every position mod 4, rows and reference
        assert {(b, k % 4) for r in rows for k, b in enumerate(r)} >= {(b, j) for b in range(1, 128)}
    assert set(ref) >= set(range(1, 128)) - {0x20}
    assert all(0 < b < 128 for r in rows + [ref] for b in r)
    # the restatement takes the reference as the program builds it, in upper case; the device gets it as it is here and upper-cases it
    clusters, scores = CL.rs_cluster(ref.upper(), rows, [0] * len(rows), 0, 0, 3, 1)
    assert ref != ref.upper()
    assert sorted(len(m) for _, m in clusters) == [2, 3, 3, 3, 3]               # the cases of one text are one cluster, nothing else joins
    up = [r.upper() for r in rows]
    r0 = sum(a != b for a, b in zip(up[0], ref.upper()))
    assert [s[0] for (m, _), s in zip(clusters, scores.tolist()) if m == 0] == [r0]
    # '`' '{' 0x7f and the like differ from '@' '[' 0x5f: 2 x (127 - 2 x 26 letters - 0x20) sites, plus the filler
    assert r0 >= 2 * (127 - 53)


# ----------------------------------------------------------------------------------------------------------- D: packed pushes
def test_group_d_shapes():
    assert {n for n, _ in E.D_SHAPES} == {1, 16, 17, 127, 128, 129, 2047, 2048, 2049, 4097}
    assert {k for n, k in E.D_SHAPES if n == 129} == {k for n, k in E.D_SHAPES if n == 2049} == {1, 63, 64, 65, 130}
    assert all((n, 65) in E.D_SHAPES for n, _ in E.D_SHAPES)
    for nchar, n in E.D_SHAPES:
        seqs = E.group_d_rows(nchar, n)
        assert len(seqs) == n and all(len(s) == nchar for s in seqs)
        pk = E.Packed(seqs)
        assert pk.planes.shape == ((n + 63) // 64, P.tile_bytes(nchar))
        hidden = bytes.maketrans(P.EXCEPTIONS, b"N" * len(P.EXCEPTIONS))
        assert pk.bare() == [t.translate(hidden) for t in pk.text]


@pytest.mark.parametrize("cut", [0xFFFFFF, 5])
def test_group_d_runs_decide(cut):
    rows = E.run_rows()
    specs = E.run_specs()
    pk = E.Packed(rows, cut=cut)
    bare = pk.bare()
    for k in range(len(specs)):
        assert bare[2 * k] != rows[2 * k] and bare[2 * k] == bare[2 * k + 1] == rows[2 * k + 1]
        n_rec = int(pk.off[2 * k + 1] - pk.off[2 * k])
        assert n_rec == sum((ln + cut - 1) // cut for _, ln, _ in specs[k]) and pk.off[2 * k + 2] == pk.off[2 * k + 1]
    per_row = np.diff(pk.off.astype(np.int64))
    assert per_row.max() >= 9                                                  # more runs in one row than the kernel has waves
    lens = (pk.exc[:, 1] >> 8).tolist()
    starts = pk.exc[:, 0].tolist()
    if cut == 5:
        assert max(lens) == 5 and per_row.max() > 200
    else:
        assert {(s % 4, ln) for s, ln in zip(starts, lens)} >= {(o, ln) for o in range(4) for ln in range(1, 10)}
        assert 257 in lens and 1027 in lens
    assert any(s + ln == E.RUNS_NCHAR for s, ln in zip(starts, lens))
    ref = rows[1].replace(b"N", b"A")
    for n_queues in (1, 3):
        q = CL.round_robin([len(rows)], n_queues)
        want = CL.rs_cluster(ref, rows, q, 0, 0, 1, n_queues)
        blind = CL.rs_cluster(ref, bare, q, 0, 0, 1, n_queues)
        assert len(want[0]) == len(rows)                                       # every run keeps its row apart from the twin
        assert blind[0] != want[0] and len(blind[0]) < len(want[0])
