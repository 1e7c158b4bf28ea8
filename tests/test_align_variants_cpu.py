"""`uvaialign --variants / --qc` without a GPU: the numpy restatement of the specification (tests/align_variants.py) against rows written by
hand, the restatement over the oracle's rows of the pools of tests/align_insertions.py -- they hold a substitution next to an insertion,
deletion runs, leading gaps and N runs, so the device test through the aligner does not pass vacuously --, the entries the header declares
and the library exports, and what the command refuses before it touches a GPU or opens a file."""
import ctypes
import os
import re
import subprocess

import align_insertions as AI
import align_variants as AV
from uvaia_amd import align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
NEW = ["uvaia_align_set_variants", "uvaia_align_variant_counts", "uvaia_align_fetch_variants", "uvaia_align_variants_of", "uvaia_align_variants_ms"]
A, C, G, T = (ord(c) for c in "ACGT")


def test_the_restatement_on_rows_written_by_hand():
    #      site 0         1         2
    #           0123456789012345678901234
    ref = b"ACGTACGTACGTACGTACGTNCGTA"
    row = b"--GTTCG---GNACRTa?GTACG--"
    recs, qc = AV.restate_row(row, ref)
    assert recs == [(0, 2, "D", 0, 0), (4, 1, "S", A, T), (7, 3, "D", 0, 0), (20, 1, "S", ord("N"), A), (23, 2, "D", 0, 0)]
    #   matches at sites 2 3 5 6 10 12 13 15 18 19 21 22; N at 11; R a ? at 14 16 17
    assert dict(zip(AV.QC_FIELDS, qc)) == dict(matches=12, substitutions=2, deletion_runs=3, deleted_sites=7, unknown_sites=1, other_sites=3, first_site=2, last_site=22)
    assert qc[0] + qc[1] + qc[3] + qc[4] + qc[5] == len(ref)
    # neighbouring substitutions are not merged; a run that is the whole row; the reference itself
    assert AV.restate_row(b"TTGT", b"ACGT")[0] == [(0, 1, "S", A, T), (1, 1, "S", C, T)]
    assert AV.restate_row(b"----", b"ACGT") == ([(0, 4, "D", 0, 0)], (0, 0, 1, 4, 0, 0, 4, -1))
    assert AV.restate_row(b"ACGT", b"ACGT") == ([], (4, 0, 0, 0, 0, 0, 0, 3))
    # two runs one base apart stay two; lower case and N opposite anything are no substitution; a base opposite a lower-case byte is one
    assert AV.restate_row(b"-C-T", b"ACGT")[0] == [(0, 1, "D", 0, 0), (2, 1, "D", 0, 0)]
    assert AV.restate_row(b"aNGT", b"ACGT") == ([], (2, 0, 0, 0, 1, 1, 0, 3))
    assert AV.restate_row(b"ACGT", b"aCGT")[0] == [(0, 1, "S", ord("a"), A)]
    recs, qcs = AV.restate([b"ACGA", b"ACGT", b"-CGT"], b"ACGT")
    assert recs == [(0, 3, 1, "S", T, A), (2, 0, 1, "D", 0, 0)] and [q[:3] for q in qcs] == [(3, 1, 0), (4, 0, 0), (3, 0, 1)]


def test_the_edge_rows_hold_what_they_are_named_for():
    names, rows = AV.edge_rows()
    ref = AV.edge_ref()
    assert len(rows) >= 17 and all(len(r) == AV.EDGE_LEN for r in rows)
    got = {n: AV.restate_row(r, ref) for n, r in zip(names, rows)}
    assert [r[0] for r in got["S at lane and round edges"][0]] == [0, 15, 16, 1023, 1024, 2049]
    assert [r[0] for r in got["S at all 16 sites of one lane"][0]] == list(range(48, 64))
    assert [r[0] // 16 for r in got["one S in every lane of a round"][0]] == list(range(64))
    for name, a, b in (("D [14,17)", 14, 17), ("D [1020,1031)", 1020, 1031), ("D [0,5)", 0, 5), ("D [2045,2050)", 2045, 2050), ("D of 1500 from 300", 300, 1800),
                       ("D over the whole second round", 1000, 2049), ("gaps only", 0, 2050)):
        assert got[name][0] == [(a, b - a, "D", 0, 0)], name
    assert got["gaps only"][1] == (0, 0, 1, 2050, 0, 0, 2050, -1)
    assert [(r[0], r[1]) for r in got["two runs one base apart"][0]] == [(100, 5), (106, 4)]
    assert [(r[0], r[1]) for r in got["single-site runs at 15 and 1023"][0]] == [(15, 1), (1023, 1)]
    assert [(r[0], r[1]) for r in got["single-site runs at 16 and 1024"][0]] == [(16, 1), (1024, 1)]
    assert [(r[0], r[2]) for r in got["S directly before and after a run"][0]] == [(15, "S"), (16, "D"), (17, "S"), (199, "S"), (200, "D"), (210, "S"), (1023, "S"), (1024, "D"), (1030, "S")]
    qc = got["N, R, a, ? and other bytes"][1]
    assert qc[4] == 102 and qc[5] == 7 and qc[1] == 0 and qc[2] == 1
    assert got["gaps but for one site"][1][6:] == (1024, 1024)
    for name in ("the reference", "nothing-1", "nothing-2", "nothing-3"):     # rows without records between rows with records
        assert got[name] == ([], (2050, 0, 0, 0, 0, 0, 0, 2049))
    # a base opposite a reference byte N is a substitution: every row that keeps the reference's bases has two
    recs, qc = AV.restate_row(rows[0], AV.edge_ref_with_n())
    assert [(r[0], r[3]) for r in recs] == [(777, ord("N")), (1024, ord("N"))] and qc[:2] == (2048, 2)


def test_the_offsets_case():
    ref, rows = AV.offsets_case()
    recs, qcs = AV.restate(rows, ref)
    per_row = [q[1] + q[2] for q in qcs]
    assert len(rows) == 2100 and all(n == 0 for n in per_row[0::3]) and all(1 <= n <= 40 for n in per_row[1::3] + per_row[2::3])
    assert set(per_row[1::3]) == set(range(1, 41))                          # 40 records: every site of a row
    assert sum(per_row) == len(recs) and any(q[2] > 3 for q in qcs)
    for n in (7, 16, 1024):
        ref, rows = AV.small_case(n, n)
        recs, qcs = AV.restate(rows, ref)
        assert (2, n - 2, 2, "D", 0, 0) in recs and (1, 0, n, "D", 0, 0) in recs and (5, n - 1, 1, "D", 0, 0) in recs, n


def _pool_records(name):
    pool = AI.pool_named(name)
    _, rows = AV.oracle_rows(pool)
    _, _, _, table = AI.expected(pool)
    return pool, rows, AV.restate(rows, pool.ref), table


def test_the_oracles_rows_hold_a_substitution_next_to_an_insertion():
    pool, rows, (recs, qcs), table = _pool_records("I-substitutions")
    assert AI.rle(AI.answer(pool, pool.seqs[0])[1]) == "300M2X2M1X2I395M"
    assert [(r[1], r[3]) for r in recs] == [(300, "S"), (301, "S"), (304, "S")]
    assert [(r, len(b)) for _, r, _, b in table] == [(305, 2)]              # the insertion lies right of the last substitution
    assert qcs[0][:4] == (697, 3, 0, 0)


def test_the_oracles_rows_hold_deletion_runs_leading_gaps_and_n_runs():
    seen = dict(runs=0, leading=0, trailing=0, unknown=0, subs=0, both=0)
    for name in AI.POOL_NAMES:
        if name == AI.long_pool().name:
            continue
        pool, rows, (recs, qcs), table = _pool_records(name)
        for q in qcs:
            assert q[0] + q[1] + q[3] + q[4] + q[5] == len(pool.ref), name
            seen["runs"] += q[2]
            seen["leading"] += q[2] > 0 and 0 < q[6] < len(pool.ref)
            seen["trailing"] += q[2] > 0 and -1 < q[7] < len(pool.ref) - 1
            seen["unknown"] += q[4] > 60
            seen["subs"] += q[1]
            seen["both"] += q[1] > 0 and q[2] > 0
    assert all(v > 0 for v in seen.values()), seen


def test_the_long_pool_is_more_than_64_rounds():
    pool = AI.long_pool()
    _, rows = AV.oracle_rows(pool)
    assert len(pool.ref) > 64 * 1024 and len(rows[0]) == len(pool.ref)
    recs, qcs = AV.restate(rows, pool.ref)
    assert qcs[0][0] + qcs[0][1] + qcs[0][3] + qcs[0][4] + qcs[0][5] == len(pool.ref)


def test_the_command_line_case():
    ref, names, seqs, dropped = AV.cli_case()
    var, qc = AV.cli_tables(ref, names, seqs, dropped)
    v, q = var.split(b"\n"), qc.split(b"\n")
    assert v[0] == b"sequence,kind,ref_pos,length,ref,alt" and q[0].startswith(b"sequence,length,score,matches,substitutions,deletions,deleted_sites,insertions,")
    assert len(q) == 1 + (len(names) - len(dropped)) + 1 and not any(d.encode() in var + qc for d in dropped)
    kinds = [ln.split(b",")[-5] for ln in v[1:-1]]                          # (names hold a comma: fields are counted from the right)
    assert kinds.count(b"I") == 29 and kinds.count(b"S") >= 6 and kinds.count(b"D") >= 4
    mine = [ln for ln in v[1:-1] if ln.startswith(names[-1].encode() + b",")]
    assert [ln.split(b",")[-5] for ln in mine].count(b"D") >= 2 and [ln.split(b",")[-5] for ln in mine].count(b"S") == 3
    # within a sequence by ref_pos, the I first where an I and another record share it
    for name in names:
        rows = [ln.split(b",")[-5:] for ln in v[1:-1] if ln.startswith(name.encode() + b",")]
        key = [(int(r[1]), 0 if r[0] == b"I" else 1) for r in rows]
        assert key == sorted(key), name
    # S lines carry ref and alt, D lines neither, I lines the bases in alt
    for ln in v[1:-1]:
        kind, pos, n, a, b = ln.split(b",")[-5:]
        assert (kind == b"S" and n == b"1" and len(a) == 1 and len(b) == 1 and a != b) or (kind == b"D" and a == b == b"") or (kind == b"I" and a == b"" and len(b) == int(n)), ln
    # (with the command's fixed penalties no optimal alignment puts an insertion directly left of a substituted or deleted site -- the
    # backtrace takes the mismatch first, and an insertion next to a deletion costs more than mismatches --, so the rule "I first at equal
    # ref_pos" decides nothing in this case; the sort above holds it all the same)


def test_the_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "uvaia_align.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "uvaia_amd", "lib", "libuvaia_gpu.so"))
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header) and s in align.SYMBOLS and hasattr(lib, s), s
    for t in ("uvaia_align_variant", "uvaia_align_row_qc"):
        assert re.search(r"typedef struct \{[^}]*\} %s;" % t, header), t
    assert align.VARIANT_DTYPE.itemsize == 16 and align.QC_DTYPE.itemsize == 32 and align.QC_DTYPE.names == AV.QC_FIELDS
    # every entry says which lines of the reference it extends
    for s in NEW:
        at = header.index(s + " (")
        assert "src/align.c:366-390" in header[header.rindex("/*", 0, at):at], s


def _refused(cmd, word, absent):
    """tests/test_compact_encode_cpu.py: refused on its own grounds, not for the missing GPU, and no output file left"""
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0, cmd
    assert word in r.stderr, (cmd, r.stderr[-2000:])
    assert b"HIP device" not in r.stderr, (cmd, r.stderr[-2000:])
    for p in absent:
        assert not os.path.exists(p), (cmd, p)


def test_the_command_refuses_tables_that_share_a_file(tmp_path):
    ref = tmp_path / "ref.fa"
    ref.write_bytes(b">ref\n" + b"ACGT" * 50 + b"\n")
    seqs = tmp_path / "s.fa"
    seqs.write_bytes(b">s0\n" + b"ACGT" * 50 + b"\n")
    t, u = str(tmp_path / "t.csv"), str(tmp_path / "u.csv")
    stem, db = str(tmp_path / "out"), str(tmp_path / "out.uvdb")
    head = [UVAIALIGN, "-r", str(ref)]
    every = [t, u, stem + ".aln.xz", db]
    _refused(head + ["--variants", t, "--qc", t, "-o", stem, str(seqs)], b"--variants and --qc name the same file", every)
    _refused(head + ["--insertions", t, "--variants", t, "-o", stem, str(seqs)], b"--insertions and --variants name the same file", every)
    _refused(head + ["--insertions", t, "--qc", t, "--variants", u, "-o", stem, str(seqs)], b"--insertions and --qc name the same file", every)
    _refused(head + ["--variants", stem + ".aln.xz", "-o", stem, str(seqs)], b"--variants names", every)
    _refused(head + ["--qc", stem + ".aln.xz", "-o", stem, str(seqs)], b"--qc names", every)
    _refused(head + ["--insertions", stem + ".aln.xz", "-o", stem, str(seqs)], b"--insertions names", every)
    _refused(head + ["--qc", db, "--packed", db, str(seqs)], b"--qc names", every)
    _refused(head + ["--variants", db, "--packed", db, str(seqs)], b"--variants names", every)
    _refused(head + [str(seqs), "--variants"], b"requires an argument", every)
    _refused(head + [str(seqs), "--qc"], b"requires an argument", every)


def test_help_names_the_options():
    r = subprocess.run([UVAIALIGN, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and b"--variants=<file>" in r.stdout and b"--qc=<file>" in r.stdout
    assert b"sequence,kind,ref_pos,length,ref,alt" in r.stdout and b"sequence,length,score,matches," in r.stdout
