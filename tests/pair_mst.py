"""Shared by the minimum-spanning-tree and nearest-row tests (uvaia_gpu_db_near*, uvaia_gpu_db_mst, `uvaiadist --mst`, `--nearest`): the
definitions of include/uvaia_gpu.h restated over the counters of every pair (pair_dist.oracle_counts_of), the text of both outputs, a step
model of the round protocol, and the number of tile pairs a call must skip.

dist and compared of a != b: snp c4 - c0 and c4, uvaia c3 - c2 and c3.  {a, b} is an edge iff compared >= min_compared.  Edges are ordered
by (dist, lo, hi), lo < hi: a strict total order, so the minimum spanning forest is unique -- what Kruskal builds taking edges in that
order.  near(x) = the smallest (dist(x, y), y) over the y with {x, y} an edge and comp[y] != comp[x], packed dist << 32 | y; NONE = 2^64 - 1."""
import functools

import numpy as np

import fixtures as F
import pair_dist as D
import pair_link as K

NONE = 2 ** 64 - 1
LAUNCH_ROWS, LAUNCH_COLS = 1024, 8192                # `constexpr size_t PAIRS_LAUNCH_ROWS = 1024, PAIRS_LAUNCH_COLS = 8192;` (host_pairs.inc)
ROW_TILE = {"snp": 32, "uvaia": 16}                  # rows of a tile pair: `constexpr int RT = 32;` (pairs_near_snp_kernel), PAIRS_CNT_RT
CASES = ["synth130"] + ["awkward9x%d" % n for n in D.NCHARS] + ["special129", "chains260x513", "dense130", "toy"]
TOY_NAMES = ["seq1", "seq2", "seq3"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(sequences upper case, nchar): the cases of pair_link and the reference README's three rows"""
    if name == "toy":
        return list(D.README_TOY), len(D.README_TOY[0])
    return K.case(name)


def trims_of(nchar):
    """0, 1, 33 and half the alignment, where they leave a window"""
    out = []
    for t in (0, 1, 33, nchar // 2):
        if 2 * t <= nchar and t not in out:
            out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def counts(name, trim=0):
    """the oracle's counters of every pair of a case over [trim, nchar - trim), int32 [n, n, 5], read-only"""
    c = D.oracle_counts_of(case(name)[0], trim)
    c.setflags(write=False)
    return c


def dist_compared(counts, metric):
    if metric == "snp":
        return D.snp(counts).astype(np.int64), counts[..., 4].astype(np.int64)
    return D.uvaia(counts).astype(np.int64), counts[..., 3].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the definitions
def kruskal_of(dist, is_edge):
    """[(a, b, dist)], a < b, sorted by (dist, a, b): the edges Kruskal keeps when it takes the edges in the order (dist, lo, hi)"""
    n = len(dist)
    a, b = np.nonzero(np.triu(is_edge, 1))
    order = np.lexsort((b, a, dist[a, b]))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    out = []
    for k in order.tolist():
        ra, rb = find(int(a[k])), find(int(b[k]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            out.append((int(a[k]), int(b[k]), int(dist[a[k], b[k]])))
            if len(out) == n - 1:
                break
    return out


def kruskal(counts, metric, min_compared=0):
    dist, compared = dist_compared(counts, metric)
    return kruskal_of(dist, compared >= min_compared)


def nearest_of(dist, is_edge, comp=None):
    """uint64 [n]: near(x) of every row; comp None: every row a component of its own"""
    n = len(dist)
    comp = np.arange(n) if comp is None else np.asarray(comp)
    key = (dist.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    ok = is_edge & (comp[:, None] != comp[None, :]) & ~np.eye(n, dtype=bool)
    key = np.where(ok, key, np.uint64(NONE))
    return key.min(axis=1) if n else np.zeros(0, dtype=np.uint64)


def nearest(counts, metric, min_compared=0, comp=None):
    dist, compared = dist_compared(counts, metric)
    return nearest_of(dist, compared >= min_compared, comp)


def prim_of(dist, is_edge):
    """the same forest as kruskal_of by Prim's algorithm over int64 keys dist << 42 | lo << 21 | hi, O(n) numpy work per row: for
    databases where a Python loop over every edge is too slow.  (Under a strict total order every correct algorithm finds the one forest.)"""
    n = len(dist)
    assert n < 2 ** 21 and int(dist.max(initial=0)) < 2 ** 20
    pos = np.arange(n, dtype=np.int64)
    inf = np.int64(2 ** 62)
    best = np.full(n, inf)
    done = np.zeros(n, dtype=bool)
    out = []
    for _ in range(n):
        open_ = np.where(done, inf, best)
        v = int(open_.argmin())
        if open_[v] != inf:
            k = int(open_[v])
            out.append(((k >> 21) & (2 ** 21 - 1), k & (2 ** 21 - 1), k >> 42))
        else:
            v = int(np.flatnonzero(~done)[0])           # a new tree of the forest starts at the smallest row left
        done[v] = True
        key = (dist[v].astype(np.int64) << 42) | (np.minimum(pos, v) << 21) | np.maximum(pos, v)
        best = np.minimum(best, np.where(is_edge[v] & (pos != v), key, inf))
    return sorted(out, key=lambda e: (e[2], e[0], e[1]))


def components_at(n, edges, max_dist):
    """labels (smallest member) of the components of the edges with dist <= max_dist"""
    return K.components(n, [(a, b) for a, b, d in edges if d <= max_dist])


# ---------------------------------------------------------------------------------------------------------------- the round protocol
def rounds_model(dist, is_edge, max_rounds=64):
    """(edges sorted by (dist, a, b), rounds) by uvaia_gpu_db_mst's protocol, a step at a time: per-endpoint keys near(x) under the current
    components -> per-component minimum under the edge order -> union (an edge chosen from both sides goes in once) -> comp[x] = smallest
    member; until a round adds nothing or one tree is left"""
    n = len(dist)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    edges, rounds = [], 0
    while len(edges) < n - 1:
        assert rounds < max_rounds
        comp = np.array([find(x) for x in range(n)])
        best = nearest_of(dist, is_edge, comp)
        rounds += 1
        choice = {}
        for x in range(n):
            if int(best[x]) == NONE:
                continue
            d, y = int(best[x]) >> 32, int(best[x]) & 0xFFFFFFFF
            e = (d, min(x, y), max(x, y))
            if comp[x] not in choice or e < choice[comp[x]]:
                choice[comp[x]] = e
        added = 0
        for c in sorted(choice):
            d, lo, hi = choice[c]
            a, b = find(lo), find(hi)
            if a == b:
                continue
            parent[max(a, b)] = min(a, b)
            edges.append((lo, hi, d))
            added += 1
        if not added:
            break
    return sorted(edges, key=lambda e: (e[2], e[0], e[1])), rounds


# ---------------------------------------------------------------------------------------------------------------- the text
def mst_text(names, edges, sep="\t"):
    """what `uvaiadist --mst` writes: a, b, dist per edge in the sorted order"""
    return "".join("%s%s%s%s%d\n" % (names[a], sep, names[b], sep, d) for a, b, d in edges).encode()


def nearest_text(names, best, sep="\t"):
    """what `uvaiadist --nearest` writes: sequence, nearest, dist per sequence in input order; no partner: an empty field and -1"""
    out = []
    for i, name in enumerate(names):
        k = int(best[i])
        out.append("%s%s%s-1\n" % (name, sep, sep) if k == NONE else "%s%s%s%s%d\n" % (name, sep, names[k & 0xFFFFFFFF], sep, k >> 32))
    return "".join(out).encode()


# ---------------------------------------------------------------------------------------------------------------- the counters
def tile_stats(comp, metric, rows=None, cols=None):
    """(tile pairs walked, tile pairs skipped) of one uvaia_gpu_db_near call over rows (first, n) x cols (first, n): the call is cut into
    launches of LAUNCH_ROWS x LAUNCH_COLS, launches wholly at or below the diagonal count nothing, and a tile pair (ROW_TILE rows of the
    launch x one tile of 64 database positions) is skipped iff its rows and columns inside the launch all carry one comp"""
    comp = np.asarray(comp)
    n, rt = len(comp), ROW_TILE[metric]
    r0, nr = rows or (0, n)
    c0, nc = cols or (0, n)
    walked = skipped = 0
    if not nr or not nc:
        return 0, 0
    for rb in range(r0, r0 + nr, LAUNCH_ROWS):
        band_end = min(rb + LAUNCH_ROWS, r0 + nr)
        if c0 + nc <= rb + 1:
            break
        for cb in range(c0, c0 + nc, LAUNCH_COLS):
            cols_end = min(cb + LAUNCH_COLS, c0 + nc)
            if cols_end <= rb + 1:
                continue
            for first in range(rb, band_end, rt):
                r = comp[first:min(first + rt, band_end)]
                for tile in range(cb // 64, (cols_end - 1) // 64 + 1):
                    c = comp[max(tile * 64, cb):min(tile * 64 + 64, cols_end)]
                    one = (r == r[0]).all() and (c == r[0]).all()
                    walked, skipped = walked + (not one), skipped + bool(one)
    return walked, skipped


# ---------------------------------------------------------------------------------------------------------------- larger inputs
_SET = np.zeros(256, dtype=np.uint8)                   # the set of bases behind every byte, bit 0 A .. bit 3 T: the planes of include/uvaia_gpu.h
for _ch, _s in zip(b"ACGTMRWSYKVHDB", (1, 2, 4, 8, 3, 5, 9, 6, 10, 12, 7, 11, 13, 14)):
    _SET[_ch] = _s
_MEET = np.array([[1.0 if a & b else 0.0 for b in range(16)] for a in range(16)], dtype=np.float32)


def dist_of_bytes(rows, trim, metric, block=1024):
    """(dist, compared) int64 [n, n] of a uint8 [n, nchar] array of upper-case text over [trim, nchar - trim), by matrix products per block
    of rows as pair_link.snp_links_of_bytes does it.  snp: both ACGT = M M', equal and ACGT = X X' with X the one-hot code of the four
    bases; uvaia: both valid = V V', sets intersect = (Y MEET) Y' with Y the one-hot code of the 16 sets.  Sums of 0/1 products: exact"""
    w = rows[:, trim:rows.shape[1] - trim]
    n = len(w)
    if metric == "snp":
        left = np.concatenate([(w == b) for b in b"ACGT"], axis=1).astype(np.float32)
        right = left
        mask = left.reshape(n, 4, -1).sum(axis=1)
    else:
        s = _SET[w]
        onehot = (s[:, :, None] == np.arange(16, dtype=np.uint8)[None, None, :]).astype(np.float32)
        left, right = (onehot @ _MEET).reshape(n, -1), onehot.reshape(n, -1)
        mask = (s != 0).astype(np.float32)
    dist, compared = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for a in range(0, n, block):
        cmp_ = mask[a:a + block] @ mask.T
        compared[a:a + block] = np.rint(cmp_)
        dist[a:a + block] = np.rint(cmp_ - left[a:a + block] @ right.T)
    return dist, compared


LAUNCH_CUT_N, LAUNCH_CUT_NCHAR = 2100, 129


@functools.lru_cache(maxsize=None)
def launch_cut_rows():
    """uint8 [2100, 129]: ACGT rows, more than one launch has rows -- a root with 0 .. 6 substitutions per row (many ties, some duplicates)"""
    rng = np.random.default_rng(83)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    root = np.frombuffer(F.random_acgt(LAUNCH_CUT_NCHAR, 85), dtype=np.uint8)
    rows = np.tile(root, (LAUNCH_CUT_N, 1))
    for i in range(LAUNCH_CUT_N):
        site = rng.choice(LAUNCH_CUT_NCHAR, size=int(rng.integers(0, 7)), replace=False)
        rows[i, site] = acgt[(np.searchsorted(acgt, rows[i, site]) + rng.integers(1, 4, size=len(site))) % 4]
    rows.setflags(write=False)
    return rows


SKIP_N, SKIP_NCHAR = 200, 129
SKIP_OUTSIDERS = (128, 191, 64, 63, 127, 192, 199, 0)   # lane 0 / lane 63 of a column tile, row 0 / row 31 of a row tile, the partial last tile


@functools.lru_cache(maxsize=None)
def skip_case():
    """(sequences, counters at trim 0) of 200 rows x 129 sites: four column tiles, the last one of 8 lanes"""
    seqs = D.upper(F.synth_alignment(SKIP_N, SKIP_NCHAR, seed=87)[0])
    c = D.oracle_counts_of(seqs, 0)
    c.setflags(write=False)
    return seqs, c


def skip_comp(outsider):
    """everything one family but one row"""
    comp = np.full(SKIP_N, 7, dtype=np.uint32)
    comp[outsider] = 1000
    return comp
