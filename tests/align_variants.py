"""The specification of `uvaialign --variants / --qc` (uvaia_align_set_variants, uvaia_align_variants_of of include/uvaia_align.h) restated in
numpy, the inputs the device tests run, and the files the command is expected to write.  No GPU code here.  tests/test_align_variants_cpu.py
checks the restatement by hand and shows that the inputs reach the cases, tests/test_align_variants_gpu.py runs them on the device.

A row is ref_len bytes on the reference's columns.  Bytes are taken as they are: A C G T are bases, '-' is a gap, 'N' is unknown, every other
byte is "other".  A substitution is a site whose byte is a base unlike the reference's byte; a deletion is a maximal run of gaps."""
import functools

import numpy as np

import align_edges as AE
import align_insertions as AI
import fixtures as F
import oracle_lib as O

QC_FIELDS = ("matches", "substitutions", "deletion_runs", "deleted_sites", "unknown_sites", "other_sites", "first_site", "last_site")
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def restate_row(row, ref):
    """([(ref_pos, length, kind, ref byte, alt byte)] in ascending ref_pos, the eight counts in the order of QC_FIELDS) of one row"""
    r, f = np.frombuffer(bytes(row), dtype=np.uint8), np.frombuffer(bytes(ref), dtype=np.uint8)
    assert r.size == f.size
    base, gap, unk = np.isin(r, _BASES), r == ord("-"), r == ord("N")
    oth = ~(base | gap | unk)
    sub, mat = base & (r != f), base & (r == f)
    recs = [(int(i), 1, "S", int(f[i]), int(r[i])) for i in np.flatnonzero(sub)]
    edge = np.diff(np.concatenate([[0], gap.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    recs += [(int(s), int(e - s), "D", 0, 0) for s, e in zip(starts, ends)]
    recs.sort()                                                           # (no S lies inside a run: positions are distinct)
    there = np.flatnonzero(~gap)
    qc = (int(mat.sum()), int(sub.sum()), len(starts), int(gap.sum()), int(unk.sum()), int(oth.sum()),
          int(there[0]) if there.size else r.size, int(there[-1]) if there.size else -1)
    assert qc[0] + qc[1] + qc[3] + qc[4] + qc[5] == r.size
    return recs, qc


def restate(rows, ref):
    """(records [(query, ref_pos, length, kind, ref, alt)] sorted by (query, ref_pos), counts [n rows of 8]) of a list of rows"""
    recs, qcs = [], []
    for q, row in enumerate(rows):
        rr, qc = restate_row(row, ref)
        recs += [(q,) + x for x in rr]
        qcs.append(qc)
    return recs, qcs


def records_of(rec):
    """the structured array Aligner.variants() returns, as restate() writes records"""
    return [(int(q), int(p), int(n), chr(k), int(a), int(b)) for q, p, n, k, a, b in zip(rec["query"], rec["ref_pos"], rec["length"], rec["kind"], rec["ref"], rec["alt"])]


def counts_of(qc):
    return [tuple(int(row[k]) for k in QC_FIELDS) for row in qc]


def flat(rows, pitch, pad=b"-"):
    """the rows `pitch` bytes apart in one buffer that ends with the last row's last site; what lies between rows is gaps, which would
    lengthen a run or close one late if a kernel looked at them"""
    out = bytearray()
    for i, row in enumerate(rows):
        out += row
        if i + 1 < len(rows):
            out += pad * (pitch - len(row))
    return bytes(out)


# ---- edges of the walk: 64 lanes x 16 sites = 1 024 sites a round
EDGE_LEN = 2050
EDGE_PITCHES = (EDGE_LEN, EDGE_LEN + 1, EDGE_LEN + 7)


def edge_ref():
    return F.random_acgt(EDGE_LEN, 20261301)


def _sub(row, sites):
    for i in sites:
        row[i:i + 1] = AE.other(bytes(row[i:i + 1]))


def _gap(row, a, b):
    row[a:b] = b"-" * (b - a)


@functools.lru_cache(maxsize=None)
def edge_rows():
    """(names, rows): at least 17 rows, so that with an odd pitch every start residue modulo 16 occurs"""
    ref = edge_ref()
    out = []

    def add(name, edit=None):
        row = bytearray(ref)
        if edit:
            edit(row)
        assert len(row) == EDGE_LEN
        out.append((name, bytes(row)))

    add("the reference")
    add("S at lane and round edges", lambda r: _sub(r, (0, 15, 16, 1023, 1024, 2049)))
    add("S at all 16 sites of one lane", lambda r: _sub(r, range(48, 64)))
    add("nothing-1")
    add("one S in every lane of a round", lambda r: _sub(r, [16 * lane + lane % 16 for lane in range(64)]))
    add("D [14,17)", lambda r: _gap(r, 14, 17))
    add("D [1020,1031)", lambda r: _gap(r, 1020, 1031))
    add("D [0,5)", lambda r: _gap(r, 0, 5))
    add("D [2045,2050)", lambda r: _gap(r, 2045, 2050))
    add("D of 1500 from 300", lambda r: _gap(r, 300, 1800))
    add("D over the whole second round", lambda r: _gap(r, 1000, 2049))
    add("two runs one base apart", lambda r: (_gap(r, 100, 105), _gap(r, 106, 110)))
    add("single-site runs at 15 and 1023", lambda r: (_gap(r, 15, 16), _gap(r, 1023, 1024)))
    add("single-site runs at 16 and 1024", lambda r: (_gap(r, 16, 17), _gap(r, 1024, 1025)))
    add("gaps only", lambda r: _gap(r, 0, EDGE_LEN))
    add("nothing-2")
    add("S directly before and after a run", lambda r: (_sub(r, (199, 210)), _gap(r, 200, 210), _sub(r, (1023, 1030)), _gap(r, 1024, 1030), _sub(r, (15, 17)), _gap(r, 16, 17)))

    def unknown_and_other(r):
        for i, ch in ((0, b"N"), (15, b"R"), (16, b"a"), (1023, b"?"), (1024, b"N"), (2049, b"R"), (500, b"n"), (501, b"\0"), (502, b"\xff")):
            r[i:i + 1] = ch
        r[600:700] = b"N" * 100
        _gap(r, 700, 720)                                               # a run between an N run and bases

    add("N, R, a, ? and other bytes", unknown_and_other)
    add("nothing-3")
    add("gaps but for one site", lambda r: (_gap(r, 0, 1024), _gap(r, 1025, EDGE_LEN)))
    add("gaps to the end from 1024", lambda r: _gap(r, 1024, EDGE_LEN))
    add("gaps up to 1024", lambda r: _gap(r, 0, 1024))
    rng = np.random.default_rng(20261302)
    for k in range(4):                                                   # everything at once, at random
        def mixed(r):
            for _ in range(30):
                a = int(rng.integers(0, EDGE_LEN))
                _gap(r, a, min(EDGE_LEN, a + int(rng.integers(1, 40))))
            for i in rng.integers(0, EDGE_LEN, 150):
                r[int(i):int(i) + 1] = bytes([rng.choice(np.frombuffer(b"ACGTNRa-", dtype=np.uint8))])
        add("mixed-%d" % k, mixed)
    assert len(out) >= 17
    return [n for n, _ in out], [r for _, r in out]


def edge_ref_with_n():
    """the edge reference with N at two sites: a base opposite a reference byte N is a substitution by definition"""
    ref = bytearray(edge_ref())
    ref[777:778] = b"N"
    ref[1024:1025] = b"N"
    return bytes(ref)


# ---- the offsets: more rows than a block has threads, rows without records between rows with records
def offsets_case(ref_len=40, n=2100, seed=20261303):
    """(ref, rows): every third row is the reference (no record); the others hold 1 to ref_len records"""
    ref = F.random_acgt(ref_len, seed)
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        row = bytearray(ref)
        if i % 3 == 1:                                                   # 1 .. ref_len substitutions
            k = 1 + (i // 3) % ref_len
            _sub(row, sorted(int(x) for x in rng.choice(ref_len, size=k, replace=False)))
        elif i % 3 == 2:                                                 # substitutions, runs and unknown bytes
            for j in range(ref_len):
                u = rng.random()
                if u < 0.25:
                    row[j:j + 1] = b"-"
                elif u < 0.45:
                    _sub(row, (j,))
                elif u < 0.5:
                    row[j:j + 1] = b"N"
            if restate_row(row, ref)[1][1] + restate_row(row, ref)[1][2] == 0:
                _sub(row, (i % ref_len,))
        rows.append(bytes(row))
    return ref, rows


def small_case(ref_len, seed):
    """a few rows of a short reference: the reference, gaps only, a run that reaches the end, a run from the start, substitutions at both ends"""
    ref = F.random_acgt(ref_len, seed)
    rows = [ref, b"-" * ref_len, ref[:ref_len - 2] + b"--", b"---" + ref[3:], AE.other(ref[:1]) + ref[1:ref_len - 1] + AE.other(ref[-1:]),
            b"-" + ref[1:ref_len - 1] + b"-", ref[:2] + b"N" + ref[3:]]
    return ref, rows


# ---- through the aligner: the pools of tests/align_insertions.py
def oracle_rows(pool):
    """(scores, rows) of the oracle for a pool"""
    scores, rows, _, _ = AI.expected(pool)
    return scores, rows


# ---- the command line: the case of tests/align_insertions.py and one sequence with deletions and substitutions
def cli_case():
    ref, names, seqs, dropped = AI.cli_case()
    extra = ref[10:200] + ref[230:400] + AE.other(ref[400:401]) + AE.other(ref[401:402]) + ref[402:520] + AE.other(ref[520:521]) + ref[521:640] + ref[641:]
    names = names + ["hCoV-19/seq %d|2021-0%d,x" % (len(seqs), 1 + len(seqs) % 9)]
    return ref, names, seqs + [extra], dropped


def cli_tables(ref, names, seqs, dropped):
    """(the file `uvaialign --variants` writes for the case, the file `--qc` writes)"""
    var = [b"sequence,kind,ref_pos,length,ref,alt\n"]
    qc = [b"sequence,length,score,matches,substitutions,deletions,deleted_sites,insertions,inserted_bases,unknown_sites,other_sites,first_site,last_site\n"]
    pool = AE.Pool("cli", ref, {}, ())
    for name, seq in zip(names, seqs):
        if name in dropped:
            continue
        score, cigar, _ = AI.answer(pool, seq)
        row = O.align_project(cigar, seq)
        recs, c = restate_row(row, ref)
        runs = AI.runs_of(cigar, seq)
        # one list by ref_pos; at equal ref_pos the insertion goes first: it lies left of that site
        lines = [(r, 0, b"I,%d,%d,,%s" % (r, len(b), b)) for r, _, b in runs]
        lines += [(p, 1, b"S,%d,1,%c,%c" % (p, a, b) if k == "S" else b"D,%d,%d,," % (p, n)) for p, n, k, a, b in recs]
        for _, _, text in sorted(lines):
            var.append(name.encode() + b"," + text + b"\n")
        qc.append(b"%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n" % (name.encode(), len(seq), score, c[0], c[1], c[2], c[3], len(runs), sum(len(b) for _, _, b in runs), c[4], c[5], c[6], c[7]))
    return b"".join(var), b"".join(qc)
