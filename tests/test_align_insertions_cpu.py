"""The inputs of tests/align_insertions.py on the CPU: the oracle's CIGARs reach the cases the insertion records are tested at on the device
(leading runs around the backtrace's strokes of 64, twenty runs in one query, a run inside a homopolymer, a run next to substitutions, runs
at the reference's end, a run abutting a deletion), the runs spliced into the oracle's row give every query back, and `uvaialign` refuses
`--insertions` without a file name before it looks for a GPU."""
import os
import subprocess

import pytest

import align_edges as AE
import align_insertions as AI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")


def _cigars(pool):
    return [AI.rle(AI.answer(pool, q)[1]) for q in pool.seqs]


def _named(name):
    return AI.pool_named(name)


@pytest.mark.parametrize("tag", ["", "-complete"])
def test_leading_runs_are_the_first_operation(tag):
    assert _cigars(_named("I-leading" + tag)) == ["%dI700M" % n for n in AI.LEADING]
    # the inputs of pool E that put junk in front of the reference start with a match (junk[0] == ref[0]): the run is the second operation
    ref, junk = AI.e_ref(), AI.e_junk()
    assert junk[0] == ref[0]
    pool = AE.Pool("E" + tag, ref, dict(min_wavefront_length=0) if tag else {}, tuple(junk[:n] + ref for n in AE.E_GAPS))
    assert _cigars(pool) == ["1M%dI699M" % n for n in AE.E_GAPS]


@pytest.mark.parametrize("tag", ["", "-complete"])
def test_many_runs_homopolymer_and_substitutions(tag):
    (c,) = _cigars(_named("I-many" + tag))
    assert c == "30M1I" * 20 + "100M"
    _, _, _, table = AI.expected(_named("I-many" + tag))
    assert [(q, r, s, len(b)) for q, r, s, b in table] == [(0, 30 * (i + 1), 31 * i + 30, 1) for i in range(20)]
    assert _cigars(_named("I-homopolymer" + tag)) == ["110M3I100M"]
    assert _cigars(_named("I-substitutions" + tag)) == ["300M2X2M1X2I395M"]


@pytest.mark.parametrize("tag", ["", "-complete"])
def test_pool_e(tag):
    pool = _named("E" + tag)
    _, _, _, table = AI.expected(pool)
    assert len({q for q, *_ in table}) == 20
    assert max(len(b) for *_, b in table) == 300
    assert sum(1 for _, r, _, _ in table if r == len(pool.ref)) == 7
    one = _named("E-one-site" + tag)
    cig = dict(zip(one.seqs, _cigars(one)))
    assert cig[b"CA"] == "1I1M" and cig[b"CG"] == "1X1I"
    empty = pool.seqs.index(b"")
    assert not [t for t in table if t[0] == empty]


def test_pools_c():
    pool = _named("C-ring-edge")
    _, _, _, table = AI.expected(pool)
    assert [(q, r, len(b)) for q, r, _, b in table] == [(0, 300, 100), (1, 300, 100), (1, 1400, 3)]
    for seq in pool.seqs:                                                                # the run of 100 abuts a deletion
        cigar = AI.answer(pool, seq)[1]
        at = cigar.index(b"I")
        assert cigar[at:at + 100] == b"I" * 100 and (cigar[at - 1:at] == b"D" or cigar[at + 100:at + 101] == b"D"), AI.rle(cigar)[:60]
    _, _, _, table = AI.expected(_named("C-x1-o0-e1"))
    assert [(r, len(b)) for q, r, _, b in table if q == 1] == [(1400, 1), (1401, 2)]


@pytest.mark.parametrize("name", AI.POOL_NAMES)
def test_runs_spliced_into_the_row_give_the_query_back(name):
    pool = _named(name)
    _, rows, _, table = AI.expected(pool)
    for q, seq in enumerate(pool.seqs):
        runs = [(r, s, b) for qq, r, s, b in table if qq == q]
        assert [r for r, _, _ in runs] == sorted({r for r, _, _ in runs}), (name, q)          # distinct, ascending
        assert all(0 <= r <= len(pool.ref) and seq[s:s + len(b)] == b and len(b) > 0 for r, s, b in runs), (name, q)
        assert AI.splice(rows[q], runs) == seq, (name, q)


def test_the_long_query_keeps_its_tail():
    pool = AI.long_pool()
    assert len(pool.seqs[0]) == 65700
    _, _, _, table = AI.expected(pool)
    assert sum(len(b) for *_, b in table) == 100


def test_the_command_line_case():
    ref, names, seqs, dropped = AI.cli_case()
    table = AI.cli_table(ref, names, seqs, dropped)
    lines = table.split(b"\n")
    assert lines[0] == b"sequence,ref_pos,length,bases" and len(lines) == 1 + 29 + 1       # ten sequences with runs, one of them with twenty
    assert not any(d.encode() in table for d in dropped)
    assert names[4].encode() not in table                              # the reference itself: no insertion, no line


def test_insertions_without_a_file_name_is_refused_before_a_gpu_is_touched(tmp_path):
    (tmp_path / "ref.fa").write_bytes(b">r\nACGT\n")
    r = subprocess.run([UVAIALIGN, "-r", str(tmp_path / "ref.fa"), str(tmp_path / "ref.fa"), "--insertions"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1
    assert b"HIP device" not in r.stdout + r.stderr
    assert b"--insertions" in r.stderr and b"requires an argument" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([UVAIALIGN, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and b"--insertions=<file>" in r.stdout and b"sequence,ref_pos,length,bases" in r.stdout
