"""Inputs and expected tables for the insertion runs of `uvaialign --insertions` (uvaia_align_set_insertions, include/uvaia_align.h).  The
CIGAR of the CPU restatement (O.wfa_align) is the specification: an insertion run is a maximal stretch of `I` operations; ref_pos counts the
M / X / D operations before it, seq_pos the M / X / I operations before it.  No GPU code here.  tests/test_align_insertions_cpu.py shows that
the oracle reaches the cases, tests/test_align_insertions_gpu.py runs them on the device."""
import functools

import align_edges as AE
import fixtures as F
import oracle_lib as O


def runs_of(cigar, seq):
    """[(ref_pos, seq_pos, bases)] of one query, in the CIGAR's order (ascending ref_pos)"""
    out, r, s, i, n = [], 0, 0, 0, len(cigar)
    while i < n:
        op = cigar[i:i + 1]
        if op == b"I":
            j = i
            while j < n and cigar[j:j + 1] == b"I":
                j += 1
            out.append((r, s, seq[s:s + j - i]))
            s += j - i
            i = j
            continue
        if op in (b"M", b"X"):
            r += 1
            s += 1
        elif op == b"D":
            r += 1
        else:
            raise ValueError(op)
        i += 1
    return out


def splice(row, runs):
    """the query back from its row on the reference's columns and its insertion runs"""
    out, at = [], 0
    for ref_pos, _, bases in runs:
        out.append(row[at:ref_pos].replace(b"-", b""))
        out.append(bases)
        at = ref_pos
    out.append(row[at:].replace(b"-", b""))
    return b"".join(out)


def rle(cigar):
    out, i = [], 0
    while i < len(cigar):
        j = i
        while j < len(cigar) and cigar[j] == cigar[i]:
            j += 1
        out.append("%d%s" % (j - i, chr(cigar[i])))
        i = j
    return "".join(out)


@functools.lru_cache(maxsize=None)
def _answer(ref, seq, kw):
    score, cigar, cells, _ = O.wfa_align(ref, seq, **dict(kw))
    return score, cigar, cells


def answer(pool, seq):
    """(score, CIGAR, cells) of the oracle for one query of a pool"""
    return _answer(pool.ref, seq, tuple(sorted(AE.oracle_kw(pool.opts).items())))


def expected(pool):
    """(scores, rows, cells in all, table): table = [(query, ref_pos, seq_pos, bases)] sorted by (query, ref_pos), as Aligner.insertions gives it"""
    scores, rows, cells, table = [], [], 0, []
    for q, seq in enumerate(pool.seqs):
        score, cigar, c = answer(pool, seq)
        scores.append(score)
        rows.append(O.align_project(cigar, seq))
        cells += c
        table += [(q, r, s, b) for r, s, b in runs_of(cigar, seq)]
    return scores, rows, cells, table


# ---- the inputs this feature adds, on the reference of pool E
LEADING = (1, 2, 63, 64, 65, 300)


def e_ref():
    return F.random_acgt(AE.E_LEN, 20261207)


def e_junk():
    return F.random_acgt(300, 20261208)


def leading_query(n):
    """n characters in front of the reference, the first of them unlike the reference's first: the run is the CIGAR's first operation"""
    ref, junk = e_ref(), e_junk()
    return AE.other(ref[:1]) + junk[1:n] + ref


def many_runs_query():
    ref = e_ref()
    return b"".join(ref[i:i + 30] + AE.other(ref[i + 30:i + 31]) for i in range(0, 600, 30)) + ref[600:]


def next_to_substitutions_query():
    ref = e_ref()
    return ref[:300] + b"GATTACA" + ref[305:]


@functools.lru_cache(maxsize=None)
def group_new():
    ref = e_ref()
    hp_ref = F.random_acgt(100, 7) + b"A" * 10 + F.random_acgt(100, 8)
    hp_q = hp_ref[:100] + b"A" * 13 + hp_ref[110:]
    out = []
    for complete in (False, True):
        opts = dict(min_wavefront_length=0) if complete else {}
        tag = "-complete" if complete else ""
        out.append(AE.Pool("I-leading" + tag, ref, opts, tuple(leading_query(n) for n in LEADING)))
        out.append(AE.Pool("I-many" + tag, ref, opts, (many_runs_query(),)))
        out.append(AE.Pool("I-homopolymer" + tag, hp_ref, opts, (hp_q,)))
        out.append(AE.Pool("I-substitutions" + tag, ref, opts, (next_to_substitutions_query(),)))
    return out


def many_runs_pool():
    return group_new()[1]


@functools.lru_cache(maxsize=None)
def long_pool():
    """the last query of pool A: the reference and 100 characters more, 65 700 in all -- its offsets never fit 16 bits"""
    (a,) = AE.group_a()
    return AE.Pool("A-longer-than-the-reference", a.ref, a.opts, (a.seqs[-1],))


def small_pools():
    """every pool but the long one, by name"""
    pools = AE.group_e(False) + [AE.Pool(p.name + "-complete", p.ref, p.opts, p.seqs) for p in AE.group_e(True)]
    for name in AE.C_NAMES:
        pools += AE.group_c(name)
    pools += AE.group_b_outside()
    pools += group_new()
    return pools


def all_pools():
    return small_pools() + [long_pool()]


POOL_NAMES = [p.name for p in all_pools()]


def pool_named(name):
    return all_pools()[POOL_NAMES.index(name)]


CLI_AMBIG_R = "0.3"


# ---- the command line: reference E, about a dozen sequences from the inputs above, two that the length filter drops
def cli_case():
    """(reference, names, sequences, names the length filter drops).  Sequence 12 is 40 % N with an insertion of five: `-a 0.5` aligns it,
    `--packed -A 0.3` (CLI_AMBIG_R) does not pack it, and its insertion is listed all the same."""
    ref, junk = e_ref(), e_junk()
    n_rich = AE.n_run(ref, 100, 280)
    seqs = [leading_query(1), leading_query(65), many_runs_query(), next_to_substitutions_query(), ref, junk[:2] + ref, ref[:350] + junk[:64] + ref[350:], ref + junk[:300],
            ref[:350] + ref[414:], ref[:200] + b"N" * 64 + AE.other(ref[264:269]) + ref[264:], ref[:100], leading_query(300), n_rich[:500] + junk[:5] + n_rich[500:], ref + ref]
    names = ["hCoV-19/seq %d|2021-0%d,x" % (i, 1 + i % 9) for i in range(len(seqs))]      # (a comma: names are written raw)
    dropped = [names[10], names[13]]
    assert 3 * len(seqs[10]) < 2 * len(ref) and 2 * len(seqs[13]) > 3 * len(ref)
    return ref, names, seqs, dropped


def cli_table(ref, names, seqs, dropped):
    """the file `uvaialign --insertions` writes for the case"""
    lines = [b"sequence,ref_pos,length,bases\n"]
    pool = AE.Pool("cli", ref, {}, ())
    for name, seq in zip(names, seqs):
        if name in dropped:
            continue
        _, cigar, _ = answer(pool, seq)
        for r, _, b in runs_of(cigar, seq):
            lines.append(b"%s,%d,%d,%s\n" % (name.encode(), r, len(b), b))
    return b"".join(lines)
