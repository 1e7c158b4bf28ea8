"""Inputs that make the edges of the uvaiaclust kernels (uvaia_amd/csrc/uvaia_cluster.hip) decide the answer: a queue whose medoid list
outgrows the part kept in LDS, comparison windows that start and end at every kind of site, rows for the distance-to-reference pass and
packed pushes of awkward shapes.  Deterministic and seeded; no GPU code here.  tests/test_cluster_edges_cpu.py shows on the restatement
that every input does what it is built for, tests/test_cluster_edges_gpu.py runs them on the device."""
import numpy as np

import fixtures as F
import packed_lib as P
from uvaia_amd import cluster

_NEXT = np.arange(256, dtype=np.uint8)
_ALT = np.arange(256, dtype=np.uint8)
for _a, _b, _c in zip(b"ACGT", b"CGTA", b"GTAC"):
    _NEXT[_a], _ALT[_a] = _b, _c


def sub(row, sites, table=_NEXT):
    """row with another letter at these sites (A -> C -> G -> T -> A; _ALT: two steps)"""
    a = np.frombuffer(row, dtype=np.uint8).copy()
    idx = np.asarray(list(sites), dtype=np.int64)
    a[idx] = table[a[idx]]
    return a.tobytes()


# ------------------------------------------------------------------------------------- A: more medoids than the LDS part of the list
LDS_ST = 14336          # uvaia_cluster.hip's LDS_ST: the stored distances kept in LDS; move this group with it
A_NCHAR = 14600
A_PLAIN = 14536         # rows 0 .. 14535: the reference with sites [0, i) substituted, r = i
# (slot the row takes, r, shift): the substituted stretch is [shift, shift + r): same r as plain row r, other content
A_EXTRAS = [(14296, 101, 3), (14333, 5000, 2), (14335, 139, 4), (14336, 14290, 5), (14338, 177, 6), (14340, 9001, 7), (14386, 14350, 8), (14400, 215, 9)]
A_PUSHES = (9000, 14420)        # rows per call end here: the last call starts with more than LDS_ST medoids in the queue


def group_a():
    """(reference, rows, queues, dict of the ordinals of the rows the test names).  dist = 0, trim = 0, n_score = 1, one queue."""
    ref = F.random_acgt(A_NCHAR, 20261101)
    r = np.frombuffer(ref, dtype=np.uint8)
    flipped = _NEXT[r]
    site = np.arange(A_NCHAR)
    lo, hi = [], []                                         # substituted stretch of every row, in push order
    extras = {slot: (rr, k) for slot, rr, k in A_EXTRAS}
    named, i = {"extras": []}, 0
    while i < A_PLAIN or len(lo) in extras:
        if len(lo) in extras:                               # every row so far founded a cluster: the next slot is the next ordinal
            rr, k = extras[len(lo)]
            named["extras"].append(len(lo))
            lo.append(k); hi.append(k + rr)
        else:
            lo.append(0); hi.append(i)
            i += 1
    named["plain_global"] = len(lo) - 20                    # a plain row far beyond LDS_ST
    named["dup_plain"] = len(lo)
    lo.append(lo[named["plain_global"]]); hi.append(hi[named["plain_global"]])
    named["dup_extra"] = len(lo)                            # its ring hit (plain row 14350) and its medoid (slot 14386) are both global
    lo.append(8); hi.append(8 + 14350)
    named["late_founder"] = len(lo)                         # ring hit in LDS (plain row 50), then every stored-1 medoid, founds
    lo.append(11); hi.append(11 + 50)
    lo, hi = np.array(lo)[:, None], np.array(hi)[:, None]
    rows = np.where((site[None, :] >= lo) & (site[None, :] < hi), flipped[None, :], r[None, :])
    seqs = [rows[k].tobytes() for k in range(len(rows))]
    return ref, seqs, [0] * len(seqs), named


# ------------------------------------------------------------------------------------------------------------- B: window edges
B_NCHARS = (1, 2, 15, 16, 17, 63, 64, 65, 1000, 1024, 1025, 4097, 8200)


def _b_trims(nchar):
    out = []
    for t in (0, 1, 15, 16, 17, int(nchar / 2.1)):
        if 2 * t < nchar and t not in out:
            out.append(t)
    return out


def _b_p0s(nchar, trim):
    out = []
    for p in (0, 1, 2, 5, 16, 17, trim, trim + 1):
        if p < nchar - 2 * trim and p not in out:
            out.append(p)
    return out


def group_b_shapes(nchar):
    """the (trim, p0) of this nchar: every third pair of the product, p0 = trim + 1 (a shift beyond the trim: the window is clamped to the
    row's end) for trim 1 and 16, and whatever is then missing of the trims and of p0 = 0, 2, 17"""
    trims = _b_trims(nchar)
    out = []
    for j, trim in enumerate(trims):
        for k, p0 in enumerate(_b_p0s(nchar, trim)):
            if (j + k) % 3 == 0 or (p0 == trim + 1 and trim in (1, 16)):
                out.append((trim, p0))
    for trim in trims:
        if not any(t == trim for t, _ in out):
            out.append((trim, _b_p0s(nchar, trim)[-1]))
    for p0 in (0, 2, 17):
        if not any(p == p0 for _, p in out):
            out += [(t, p0) for t in trims if p0 in _b_p0s(nchar, t)][:1]
    return out


def group_b_case(nchar, trim, p0, dist):
    """(reference, rows) of one case, or None where dist = 1 finds no free interior site.  Row 0 is the base: the reference with one
    difference at trimmed position p0.  Every other row differs from the base at one edge site (and, for dist = 1, at one fixed interior
    site as well, so that a comparison counts 1 or 2); the last one holds another letter at the base's own difference."""
    ref = F.random_acgt(nchar, 7000 + nchar)
    hi, m, first = nchar - trim, max(0, p0 - 1), trim + p0
    edges = []
    for e in (0, trim - 1, trim, first + 1, hi - 1, hi, hi + m - 1, hi + m, nchar - 1, 4095, 4096):
        if 0 <= e < nchar and e != first and e not in edges:
            edges.append(e)
    extra = []
    if dist:
        free = [s for s in range(first + 2, hi - 1) if s not in edges] or [s for s in range(trim, hi) if s != first and s not in edges]
        if not free:
            return None
        extra = [free[len(free) // 2]]
    base = sub(ref, [first])
    rows = [base] + [sub(base, [e] + extra) for e in edges] + [sub(sub(ref, [first], _ALT), extra)]
    return ref, rows


def group_b_cases(nchar):
    """[(trim, p0, dist, reference, rows)] of this nchar"""
    out = []
    for trim, p0 in group_b_shapes(nchar):
        for dist in (0, 1):
            c = group_b_case(nchar, trim, p0, dist)
            if c:
                out.append((trim, p0, dist) + c)
    return out


def alternate(n):
    """base and twins alternating over two queues: rows of the two meet in the merge"""
    return [k % 2 for k in range(n)]


# ------------------------------------------------------------------------------------------------- C: positions, counts, bytes
C_NCHAR = 5000
C_N_SCORES = (0, 1, 3, 70)
C_TRIMS = (0, 17)


def group_c_sites(trim, n_score):
    """differing sites (absolute) of every row"""
    hi = C_NCHAR - trim
    rng = np.random.default_rng(900 + 10 * n_score + trim)
    rows = [[], [trim], [40, 42], list(range(64, 80)), list(range(trim + 16, trim + 32)), [15, 16], [trim + 15, trim + 16],
            [1023, 1024], [4095, 4096], [1023, 1024, 4095, 4096], [trim + 64 * k + 5 for k in range(70)], list(range(1015, 1035)),
            list(range(1000, 1090)), [hi - 1], [trim, hi - 1]]
    for k in (n_score - 1, n_score, n_score + 1):
        if k > 0:
            rows.append(sorted(rng.choice(np.arange(trim, hi), size=k, replace=False).tolist()))
            rows.append([trim + 1020 + 3 * j for j in range(k)])             # the same counts across the 1 024-site chunk boundary
    if trim:
        rows += [[0], [trim - 1], [hi], [C_NCHAR - 1], [0, 3, trim - 1, hi, hi + 5, C_NCHAR - 1]]        # the margins alone: r = 0, every p = -1
    return [s for k, s in enumerate(rows) if s not in rows[:k]]


def group_c(trim, n_score):
    """(reference, rows, expected [r, p...] of every row by the definition: differences inside [trim, nchar - trim), the first n_score of them)"""
    ref = F.random_acgt(C_NCHAR, 31)
    sites = group_c_sites(trim, n_score)
    rows = [sub(ref, s) for s in sites]
    want = []
    for s in sites:
        inside = sorted(x - trim for x in s if trim <= x < C_NCHAR - trim)
        want.append([len(inside)] + (inside + [-1] * n_score)[:n_score])
    return ref, rows, want


def check_group_c(clusters, scores, want, n_score):
    """the stored vectors by the definition: the first n_score differing sites of the medoid; r itself, or d + 1 = 1 after a comparison"""
    for (m, _), s in zip(clusters, scores.tolist()):
        assert s[1:1 + n_score] == want[m][1:], (m, s, want[m])
        assert s[0] in (want[m][0], 1), (m, s, want[m])
        assert s[-1] == C_NCHAR


BYTES_NCHAR = 300


def group_bytes():
    """(reference, rows): every byte 1..127 at every position mod 4 and on both sides of 16-byte boundaries, in the rows and in the reference"""
    every = bytes(range(1, 128))
    rows = []
    for j in range(4):
        s = (b"A" * j + every + b"c" * (j + 1) + every)
        s = s + b"g" * (BYTES_NCHAR - len(s))
        rows += [s, s.upper(), s.lower(), s.swapcase()]
    ref = bytes((b ^ 0x20) or b for b in rows[0])               # '@' against '`', '[' against '{', 0x5f against 0x7f, digits against controls
    rows += [ref, ref.upper(), ref.lower()]
    return ref, rows


# ----------------------------------------------------------------------------------------------------------- D: packed pushes
D_SHAPES = sorted({(nchar, 65) for nchar in (1, 16, 17, 127, 128, 129, 2047, 2048, 2049, 4097)} |
                  {(nchar, n) for nchar in (129, 2049) for n in (1, 63, 64, 65, 130)})


class Packed:
    """sequences as a packed database holds them: whole tiles and the exception runs of the upper-case text"""

    def __init__(self, seqs, cut=0xFFFFFF):
        self.text = [s.upper() for s in seqs]
        self.n, self.nchar = len(seqs), len(seqs[0])
        self.planes = P.pack_tiles(self.text, self.nchar)[0]
        self.off, self.exc = cluster.exception_runs(self.text, cut=cut)

    def bare(self):
        """what the planes alone decode to"""
        return [P.decode_reference(self.planes, i, self.nchar) for i in range(self.n)]


def group_d_rows(nchar, n):
    return P.awkward_references(n, nchar, seed=1000 + nchar + n)


RUNS_NCHAR = 1100


def run_specs():
    """runs (start, length, character) of every hand-built row"""
    ch = "-?XO."
    out = [[(40 + o, ln, ch[(o + ln) % 5])] for o in range(4) for ln in range(1, 10)]          # every start offset and length mod 4
    out.append([(200, 5, "-"), (205, 3, "?")])                                                  # touching, the boundary inside a 4-byte word
    out.append([(300, 6, "X"), (306, 4, "O"), (310, 7, ".")])
    out.append([(601, 2, "."), (603, 1, "-"), (604, 4, "?"), (608, 1, "X")])
    out.append([(401, 257, "-")])                                                               # more than one pass of the 64 lanes
    out.append([(5, 1027, "?")])
    out.append([(50 + 101 * k, 3 + k, ch[k % 5]) for k in range(9)])                            # more runs than waves
    out.append([(RUNS_NCHAR - 10, 10, "-")])                                                    # up to the last site
    out.append([(0, 1, "O"), (RUNS_NCHAR - 1, 1, ".")])
    out.append([(700, 13, "-")])                                                                # cut = 5 makes three records of it
    return out


def run_rows():
    """every run row followed by its twin with N there: the runs decide whether the two are one cluster"""
    rows = []
    for k, spec in enumerate(run_specs()):
        base = bytearray(F.random_acgt(RUNS_NCHAR, 500 + k))
        twin = bytearray(base)
        for a, ln, c in spec:
            base[a:a + ln] = c.encode() * ln
            twin[a:a + ln] = b"N" * ln
        rows += [bytes(base), bytes(twin)]
    return rows
