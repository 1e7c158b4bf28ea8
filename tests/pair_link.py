"""Shared by the single-linkage cluster tests (uvaia_gpu_db_link*, `uvaiadist --clusters`): the constructed cases, and the definition of
include/uvaia_gpu.h restated as a plain union-find over the counters of every pair (pair_dist.oracle_counts_of or plane_counts_of).

Two rows a < b are linked iff dist(a, b) <= D and compared(a, b) >= min_compared; snp: dist = c4 - c0, compared = c4 (ACGT_pair_comparisons);
uvaia: dist = c3 - c2, compared = c3 (valid_pair_comparisons).  A cluster is a connected component, its label the smallest position in it."""
import functools

import numpy as np

import fixtures as F
import pair_dist as D

CHAIN_FAMILIES = (1, 1, 2, 3, 63, 64, 65, 61)        # members per family of chains260x513
CHAIN_NCHAR = 513
SYNTH_FLOOR = 505                                    # a floor that bites on synth130: its pairs are compared over 480 .. 513 sites, half of them over fewer than 507


def _substitute(row, site):
    row[site] = b"ACGT"[(b"ACGT".index(row[site]) + 1) % 4]


@functools.lru_cache(maxsize=None)
def chains():
    """(sequences by position, family of every position, member number of every position): 260 rows of 513 sites from one ACGT root.
    Family f carries three signature substitutions of its own (two rows of different families are at least 6 apart); member k of a
    family carries the family's first k chain substitutions (neighbours 1 apart, the ends members - 1 apart).  Sites are used once.
    Positions: member 30 of each of the four large families sits in the last tile (256 .. 259); the other 256 rows, in family order,
    go to (index * 77) % 256, so that consecutive members land in different tiles."""
    root = F.random_acgt(CHAIN_NCHAR, 29)
    site = iter(np.random.default_rng(31).permutation(CHAIN_NCHAR).tolist())
    logical = []
    for f, members in enumerate(CHAIN_FAMILIES):
        base = bytearray(root)
        for _ in range(3):
            _substitute(base, next(site))
        for k in range(members):
            logical.append((bytes(base), f, k))
            _substitute(base, next(site))             # (the last one of a family is not used)
    n = len(logical)
    assert n == 260
    last_tile = [i for i, (_s, f, k) in enumerate(logical) if CHAIN_FAMILIES[f] > 60 and k == 30]
    rest = [i for i in range(n) if i not in last_tile]
    at = [None] * n
    for p, i in zip(range(256, 260), last_tile):
        at[p] = logical[i]
    for j, i in enumerate(rest):
        at[(j * 77) % 256] = logical[i]
    return [x[0] for x in at], [x[1] for x in at], [x[2] for x in at]


@functools.lru_cache(maxsize=None)
def case(name):
    """(sequences upper case, nchar): the cases of pair_dist and the constructed ones"""
    if name == "chains260x513":
        return chains()[0], CHAIN_NCHAR
    if name == "dense130":
        return [F.random_acgt(513, 37)] * 130, 513
    return D.case(name)


@functools.lru_cache(maxsize=None)
def counts(name, trim=0):
    """the oracle's counters of every pair of a case, int32 [n, n, 5], read-only"""
    c = D.oracle_counts_of(case(name)[0], trim)
    c.setflags(write=False)
    return c


def linked(counts, metric, max_dist, min_compared=0):
    """bool [n, n]: the pairs the definition links (symmetric, the diagonal included)"""
    dist = D.snp(counts) if metric == "snp" else D.uvaia(counts)
    compared = counts[..., 4] if metric == "snp" else counts[..., 3]
    return (dist <= max_dist) & (compared >= min_compared)


def components(n, pairs):
    """(labels uint32 [n], the smallest member of every row's component) by a plain union-find over (a, b) pairs"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)


def restate(counts, metric, max_dist, min_compared=0, rows=None, cols=None):
    """(labels, n_links) of the pairs row < col inside rows (first, n) x cols (first, n) (None: everything) of a square counter matrix"""
    n = counts.shape[0]
    r0, nr = rows or (0, n)
    c0, nc = cols or (0, n)
    keep = linked(counts, metric, max_dist, min_compared)
    pos = np.arange(n)
    keep = keep & (pos[:, None] < pos[None, :])
    keep[:r0] = False
    keep[r0 + nr:] = False
    keep[:, :c0] = False
    keep[:, c0 + nc:] = False
    pairs = np.argwhere(keep)
    return components(n, pairs), len(pairs)


def sizes_of(labels):
    """the size of every row's cluster"""
    _u, inverse, count = np.unique(labels, return_inverse=True, return_counts=True)
    return count[inverse]


def clusters_text(names, labels, sep="\t", min_size=1):
    """what `uvaiadist --clusters` writes: sequence, cluster (1, 2, ... in order of first member), size; clusters below min_size left out"""
    number, out = {}, []
    size = sizes_of(labels)
    for i, name in enumerate(names):
        k = number.setdefault(int(labels[i]), len(number) + 1)
        if size[i] >= min_size:
            out.append("%s%s%d%s%d\n" % (name, sep, k, sep, size[i]))
    return "".join(out).encode()


def snp_links_of_bytes(rows, trim, max_dist, block=1024):
    """the (a, b), a < b, with snp distance <= max_dist over [trim, nchar - trim) of a uint8 [n, nchar] array of upper-case text, by two
    matrix products per block of rows: both ACGT = M M', equal and ACGT = X X' with X the one-hot code of the four bases"""
    w = rows[:, trim:rows.shape[1] - trim]
    onehot = np.concatenate([(w == b) for b in b"ACGT"], axis=1).astype(np.float32)
    acgt = onehot.reshape(len(w), 4, -1).sum(axis=1)
    pairs = []
    for a in range(0, len(w), block):
        dist = acgt[a:a + block] @ acgt.T - onehot[a:a + block] @ onehot.T
        i, j = np.nonzero(dist <= max_dist)
        i += a
        pairs.append(np.stack([i[i < j], j[i < j]], axis=1))
    return np.concatenate(pairs)
