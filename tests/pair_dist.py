"""Shared by the all-pairs distance tests (uvaia_gpu_db_pairs, uvaia_gpu_db_pairs_within, uvaiadist): the cases, what the oracle's two
kernels give for every pair over the trimmed text, and the plane formulas of include/uvaia_gpu.h restated in numpy over
packed_lib.pack_tiles (no GPU needed).

Counters of a pair: 0 ACGT_matches, 1 text_matches, 2 partial_matches, 3 valid_pair_comparisons (orc_score_matches_truncated_idx with
nothing truncated), 4 ACGT_pair_comparisons (orc_score_acgt_and_valid score[1]); snp = c4 - c0 (= its score[0]), uvaia = c3 - c2."""
import ctypes as C
import functools

import numpy as np

import fixtures as F
import oracle_lib as O
import packed_lib as P

NCOUNT = 5
INT_MAX = 2 ** 31 - 1
NCHARS = (31, 32, 33, 127, 128, 129, 513)            # around a word, a word group, and several word groups with a partial last one
TRIMS = (0, 1, 31, 32, 33, "half")                   # "half": nchar // 2 (the empty or one-site window)
README_TOY = (b"AACGTTA--", b"AACG-TAM-", b"MNCGTTMC-")   # the reference README's three-sequence example (lines 307-316)


def trims_of(nchar):
    out = []
    for t in TRIMS:
        t = nchar // 2 if t == "half" else t
        if 2 * t <= nchar and t not in out:
            out.append(t)
    return out


def upper(seqs):
    """the text as the FASTA reader hands it over: upper case (the oracle compares bytes, the planes hold sets)"""
    return [bytes(s).upper() for s in seqs]


def special_rows(nchar, seed=5):
    """an all-N row, an all-'-' row, a row of partial codes only, two identical rows, and two ordinary ones"""
    rng = np.random.default_rng(seed)
    part = np.frombuffer(b"MRWSYKVHDB", dtype=np.uint8)
    a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar).tobytes()
    b = bytearray(a)
    for k in range(0, nchar, 7):
        b[k] = b"ACGT"[(b"ACGT".index(b[k]) + 1) % 4]
    return [b"N" * nchar, b"-" * nchar, part[rng.integers(0, len(part), size=nchar)].tobytes(), a, a, bytes(b)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(sequences upper case, nchar)"""
    if name == "synth130":
        return upper(F.synth_alignment(130, 513, seed=11)[0]), 513
    if name.startswith("awkward"):                    # "awkward<N>x<nchar>"
        n, nchar = (int(x) for x in name[len("awkward"):].split("x"))
        return upper(P.awkward_references(n, nchar, seed=17)), nchar
    if name.startswith("special"):
        nchar = int(name[len("special"):])
        return special_rows(nchar), nchar
    raise KeyError(name)


CPU_CASES = ["synth130"] + ["awkward9x%d" % n for n in NCHARS] + ["special129"]


@functools.lru_cache(maxsize=None)
def _idx(n):
    return (C.c_size_t * n)(*range(n))


def oracle_counts_of(seqs, trim=0):
    """int32 [n, n, 5]: the counters of every pair by the oracle's two kernels over the text [trim, nchar - trim)"""
    L = O.lib()
    n, nchar = len(seqs), len(seqs[0])
    cut = [s[trim:nchar - trim] for s in seqs]
    m = nchar - 2 * trim
    out = np.zeros((n, n, NCOUNT), dtype=np.int32)
    r4, r2 = (C.c_int * 4)(), (C.c_int * 2)()
    for i in range(n):
        for j in range(i, n):
            L.orc_score_matches_truncated_idx(cut[i], cut[j], m, INT_MAX, r4, _idx(m))
            L.orc_score_acgt_and_valid(cut[i], cut[j], m, INT_MAX, r2, _idx(m))
            assert r2[0] == r2[1] - r4[0]             # both ACGT and different = both ACGT - equal and ACGT
            out[i, j] = out[j, i] = (r4[0], r4[1], r4[2], r4[3], r2[1])
    return out


@functools.lru_cache(maxsize=None)
def oracle_counts(name, trim=0):
    c = oracle_counts_of(case(name)[0], trim)
    c.setflags(write=False)
    return c


def snp(counts):
    return counts[..., 4] - counts[..., 0]


def uvaia(counts):
    return counts[..., 3] - counts[..., 2]


def _popcount(x):
    x = x.astype(np.uint32)
    x = x - ((x >> 1) & np.uint32(0x55555555))
    x = (x & np.uint32(0x33333333)) + ((x >> 2) & np.uint32(0x33333333))
    x = (x + (x >> 4)) & np.uint32(0x0F0F0F0F)
    return ((x * np.uint32(0x01010101)) >> 24).astype(np.int64)


def window_masks(n_words, nchar, trim):
    """uint32 [n_words]: the bits of every alignment word inside [trim, nchar - trim)"""
    site = np.arange(n_words * 32)
    inside = ((site >= trim) & (site < nchar - trim)).reshape(n_words, 32)
    return (inside.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def plane_counts_of(seqs, nchar, trim=0, rows=None):
    """the same [n, n, 5] from the packed tiles alone: valid = some plane bit, ACGT = exactly one, equal and valid = four equal planes with
    one set, intersect = some plane with both bits; the window clears one side only.  rows: only the first so many rows, [rows, n, 5], or
    (first, count): only rows [first, first + count), [count, n, 5]"""
    planes, _non_n = P.pack_tiles(seqs, nchar)
    n, W4 = len(seqs), ((nchar + 31) // 32 + 3) // 4
    t = planes.reshape(-1).view(np.uint32).reshape(-1, W4, 4, 64, 4)                  # [tile, w4, plane, lane, j]
    w = t.transpose(0, 3, 2, 1, 4).reshape(-1, 4, W4 * 4)[:n]                        # [ref, plane, word]
    A, Cc, G, T = (w[:, p, :] for p in range(4))
    valid = A | Cc | G | T
    par, three = A ^ Cc ^ G ^ T, (A & Cc & (G | T)) | (G & T & (A | Cc))
    single = par & ~three
    m = window_masks(W4 * 4, nchar, trim)
    first, n_rows = (0, n) if rows is None else rows if isinstance(rows, tuple) else (0, rows)
    assert 0 <= first and first + n_rows <= n
    out = np.zeros((n_rows, n, NCOUNT), dtype=np.int32)
    for i in range(n_rows):                            # row side: cleared outside the window
        a, c, g, tt, v, s = (x[first + i] & m for x in (A, Cc, G, T, valid, single))
        equal = ~((A ^ a) | (Cc ^ c) | (G ^ g) | (T ^ tt))
        inter = (A & a) | (Cc & c) | (G & g) | (T & tt)
        out[i, :, 0] = _popcount(equal & s).sum(axis=1)
        out[i, :, 1] = _popcount(equal & valid).sum(axis=1)
        out[i, :, 2] = _popcount(inter).sum(axis=1)
        out[i, :, 3] = _popcount(valid & v).sum(axis=1)
        out[i, :, 4] = _popcount(single & s).sum(axis=1)
    return out


def dummy_query(nchar, acgt=False):
    """a query set to open an engine over (the pair counters do not depend on it)"""
    root = F.random_acgt(nchar, 3)
    q2 = bytearray(root)
    q2[nchar // 2] = b"ACGT"[(b"ACGT".index(q2[nchar // 2]) + 1) % 4]
    return O.Query([root, bytes(q2)], ["q0", "q1"], acgt=acgt)


def within_expected(counts, max_dist, metric="snp", upper=True, rows=None, cols=None, is_rectangle=False):
    """(row, col, counters) of the pairs a threshold call must list for rows (first, n) x cols (first, n), in (row, col) order; counts: the
    whole matrix, or with is_rectangle the counters of that rectangle alone"""
    r0, nr = rows or (0, counts.shape[0])
    c0, nc = cols or (0, counts.shape[1])
    rect = counts if is_rectangle else counts[r0:r0 + nr, c0:c0 + nc]
    assert rect.shape[:2] == (nr, nc)
    keep = (snp(rect) if metric == "snp" else uvaia(rect)) <= max_dist
    if upper:
        keep &= (r0 + np.arange(nr))[:, None] < (c0 + np.arange(nc))[None, :]
    return [(r0 + int(i), c0 + int(j), tuple(int(x) for x in rect[i, j])) for i, j in np.argwhere(keep)]
