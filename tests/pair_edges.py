"""Inputs that take the all-pairs kernels (kernels_pairs.inc, host_pairs.inc) to the edges their feature tests leave out, and the plain
restatements that judge them.  numpy only, deterministic and seeded; no GPU code here.  tests/test_pair_edges_cpu.py checks the builders
and the model, tests/test_pair_edges_gpu.py runs the inputs through uvaia_gpu_db_pairs, _db_pairs_within and _db_link*.

  A  the forest under contention   builders whose clusters are known by construction (dense, chain, star, bridged) at a size where one
                                   launch has more blocks than the chip has CUs, and forest_model: pairs_link_root / pairs_link_hits
                                   restated step by step under a random scheduler and stale loads (DESIGN.md 4.12's argument)
  B  stale bits in handed-in tiles dirty(): lanes past the last row and bits at and past nchar of exported tiles overwritten
  C  the launch cut                launch_rows(): the 8 200-row database of test_links_across_launches, and the uvaia links of all its
                                   pairs by matrix products (pinned to pair_dist.plane_counts_of in the CPU test)
Nothing here ever reads what an engine gave: expected values come from the construction, pair_dist.plane_counts_of, pair_link.components,
pair_link.restate and pair_link.snp_links_of_bytes."""
import collections
import functools

import numpy as np

import fixtures as F
import pair_dist as D
import pair_link as K

# ---- copies of the code's constants; each moves with the line it mirrors
LAUNCH_ROWS, LAUNCH_COLS = 1024, 8192                # `constexpr size_t PAIRS_LAUNCH_ROWS = 1024, PAIRS_LAUNCH_COLS = 8192;` (host_pairs.inc)
CONTENDED_N = 4160                                   # 65 column tiles, five row bands: 32 x 17 = 544 blocks in one launch of pairs_link_snp_kernel
CONTENDED_NCHAR = 4224                               # chain and star at CONTENDED_N: W4 = 33
SMALL_N = 260                                        # the size at which the CPU test checks every pair of a builder

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NEXT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    _NEXT[_a] = _b


def _root_row(nchar, seed):
    return np.frombuffer(F.random_acgt(nchar, seed), dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------------------------ A: builders
# Built: rows uint8 [N, nchar] by database position, logical [N] = the logical member at every position, kind, and for D in (0, 1) the
# expected labels (the smallest position of every component) and number of links, all from the construction.
Built = collections.namedtuple("Built", "rows logical kind labels links")

POSITION_MAPS = ("identity", "reversed", "mod77")


def position_map(name, n):
    """pos[i] = the database position of logical member i"""
    i = np.arange(n)
    if name == "identity":
        return i
    if name == "reversed":
        return n - 1 - i
    if name == "mod77":                               # neighbours land in different tiles and bands (77 and n must be coprime)
        assert np.gcd(77, n) == 1
        return (i * 77) % n
    raise KeyError(name)


def _placed(logical_rows, pos, kind, component, links):
    """rows by position, and the labels of {D: component id of every logical member}"""
    n = len(logical_rows)
    pos = np.asarray(pos)
    assert sorted(pos.tolist()) == list(range(n))
    rows = np.empty_like(logical_rows)
    rows[pos] = logical_rows
    logical = np.empty(n, dtype=np.int64)
    logical[pos] = np.arange(n)
    labels = {}
    for d, comp in component.items():
        comp = np.asarray(comp)
        smallest = np.full(int(comp.max()) + 1, n, dtype=np.int64)
        np.minimum.at(smallest, comp, pos)
        lab = np.empty(n, dtype=np.uint32)
        lab[pos] = smallest[comp]
        labels[d] = lab
    rows.setflags(write=False)
    return Built(rows, logical, kind, labels, links)


@functools.lru_cache(maxsize=None)
def dense(n):
    """n identical rows of 33 sites: n (n - 1) / 2 links and one cluster at every D, while the floor is met"""
    rows = np.tile(_root_row(33, 51), (n, 1))
    one = np.zeros(n, dtype=np.int64)
    return _placed(rows, np.arange(n), "dense", {0: one, 1: one}, {0: n * (n - 1) // 2, 1: n * (n - 1) // 2})


@functools.lru_cache(maxsize=None)
def chain(n, nchar, order="identity"):
    """member k carries the first k of n - 1 substitutions, every site used once: dist(i, j) = |i - j|.  Under the identity map the hooks
    make parent[i + 1] = i, a path as long as the component"""
    assert nchar >= n - 1
    site = np.random.default_rng(53).permutation(nchar)[:n - 1]
    rows = np.tile(_root_row(nchar, 55), (n, 1))
    for k in range(1, n):
        rows[k:, site[k - 1]] = _NEXT[rows[0, site[k - 1]]]
    return _placed(rows, position_map(order, n), "chain", {0: np.arange(n), 1: np.zeros(n, dtype=np.int64)}, {0: 0, 1: n - 1})


@functools.lru_cache(maxsize=None)
def star(n, nchar, hub_at):
    """logical member 0 is the hub, members 1 .. n - 1 carry one private substitution each: hub to leaf 1, leaf to leaf 2.  hub_at: the
    hub's database position, 0 or n - 1 (there every wave's first CAS lands on the same node); the leaves keep their order"""
    assert nchar >= n - 1 and hub_at in (0, n - 1)
    site = np.random.default_rng(57).permutation(nchar)[:n - 1]
    rows = np.tile(_root_row(nchar, 59), (n, 1))
    rows[np.arange(1, n), site] = _NEXT[rows[0, site]]
    pos = np.arange(n) if hub_at == 0 else np.concatenate([[n - 1], np.arange(n - 1)])
    return _placed(rows, pos, "star", {0: np.arange(n), 1: np.zeros(n, dtype=np.int64)}, {0: 0, 1: n - 1})


@functools.lru_cache(maxsize=None)
def bridged(n):
    """identical rows A at the even positions and identical rows B at the odd ones, two sites apart, 33 sites; the last position (odd, n is
    even) holds a row that differs from A at one of the two sites, 1 from both.  D = 0: three components 0, 1, n - 1; D = 1: one"""
    assert n % 2 == 0 and n >= 4
    a = _root_row(33, 61)
    b = a.copy()
    b[[7, 29]] = _NEXT[a[[7, 29]]]
    bridge = a.copy()
    bridge[7] = b[7]
    rows = np.where((np.arange(n) % 2 == 0)[:, None], a[None, :], b[None, :])
    rows[n - 1] = bridge
    comp0 = np.arange(n) % 2
    comp0[n - 1] = 2
    n_a, n_b = n // 2, n // 2 - 1
    same = n_a * (n_a - 1) // 2 + n_b * (n_b - 1) // 2
    return _placed(rows, np.arange(n), "bridged", {0: comp0, 1: np.zeros(n, dtype=np.int64)}, {0: same, 1: same + n - 1})


def distances_from(built, p):
    """int [N]: the snp distance of position p to every position, from the construction alone"""
    n = len(built.logical)
    k, me = built.logical, int(built.logical[p])
    if built.kind == "dense":
        return np.zeros(n, dtype=np.int64)
    if built.kind == "chain":
        return np.abs(k - me)
    if built.kind == "star":
        return np.where(k == me, 0, np.where((k == 0) | (me == 0), 1, 2))
    if built.kind == "bridged":
        cls = np.arange(n) % 2
        cls[n - 1] = 2
        table = np.array([[0, 2, 1], [2, 0, 1], [1, 1, 0]])
        return table[cls[p]][cls]
    raise KeyError(built.kind)


def construction_links(built, max_dist):
    """the (a, b), a < b, of positions within max_dist, from the construction alone (chain and star: the tree's edges at D = 1)"""
    assert built.kind in ("chain", "star") and max_dist == 1
    at = np.argsort(built.logical)                    # position of every logical member
    n = len(at)
    ends = np.stack([at[:-1], at[1:]], axis=1) if built.kind == "chain" else np.stack([np.full(n - 1, at[0]), at[1:]], axis=1)
    return np.sort(ends, axis=1)


def bands_reversed(n, height=64):
    """the calls of one db_link per band of `height` rows against all columns, last band first"""
    return [((r, min(height, n - r)), None) for r in range(0, n, height)][::-1]


def quadrants(n):
    half = ((0, n // 2), (n // 2, n - n // 2))
    return [(r, c) for r in half for c in half]


# ------------------------------------------------------------------------------------------------------------------ A: the argument
# pairs_link_root and pairs_link_hits (kernels_pairs.inc) restated one memory operation at a time.  A lane is a generator that yields its
# next operation and is sent the result; forest_model performs one lane's pending operation per step, the lane picked at random, so every
# interleaving of loads, compare-and-swaps and atomicMins can come up.  A load returns ANY value the cell ever held (the staleness DESIGN.md
# 4.12 allows: no coherence, no order between cells, not even within one lane); CAS and min act on the current value.
def _root(x):
    """`for (;;) { const uint32_t p = pairs_link_load(parent + x); if (p >= x) return x; x = p; }`"""
    while True:
        p = yield ("load", x)
        if p >= x:
            return x
        x = p


def _lane(col, rows, atomic_cas):
    """one lane of pairs_link_hits: `col` and its hit rows of one row tile in ascending order (`__ffs`), all < col"""
    seen = yield ("load", col)                        # `const uint32_t seen = pairs_link_load(parent + col);`
    rc = col if seen >= col else (yield from _root(seen))      # `uint32_t rc = seen >= col ? col : pairs_link_root(parent, seen);`
    for r in rows:                                    # `while (hits) { const uint32_t r = (uint32_t)__ffs((int)hits) - 1u; hits &= hits - 1u;`
        rr = yield from _root(r)                      # `uint32_t rr = pairs_link_root(parent, row_first + r);`
        while rr != rc:                               # `while (rr != rc) {`
            hi, lo = max(rr, rc), min(rr, rc)         # `const uint32_t hi = max(rr, rc), lo = min(rr, rc);`
            if atomic_cas:
                old = yield ("cas", hi, hi, lo)       # `const uint32_t old = atomicCAS(parent + hi, hi, lo);`
            else:                                     # the mutant: load, compare, store -- two steps, another lane's hook fits in between
                old = yield ("load_now", hi)
                if old == hi:
                    yield ("store", hi, lo)
            if old >= hi:                             # `if (old >= hi) { rc = lo; break; }`
                rc = lo
                break
            rr = yield from _root(old)                # `rr = pairs_link_root(parent, old);`
            rc = yield from _root(lo)                 # `rc = pairs_link_root(parent, lo);`
    if rc < seen:                                     # `if (rc < seen) atomicMin(parent + col, rc);`
        yield ("min", col, rc)


def lanes_of(edges, rng, max_lanes=3):
    """[(col, rows)]: every column's hit rows (the a of its edges (a, b), a < b) in ascending order, cut into up to max_lanes contiguous
    runs -- the lanes of different row tiles that hold the same column"""
    by_col = collections.defaultdict(set)
    for a, b in edges:
        a, b = int(min(a, b)), int(max(a, b))
        assert a != b
        by_col[b].add(a)
    lanes = []
    for col, rows in sorted(by_col.items()):
        rows = sorted(rows)
        cuts = sorted(set(rng.integers(1, len(rows), size=int(rng.integers(0, max_lanes))).tolist())) if len(rows) > 1 else []
        for a, b in zip([0] + cuts, cuts + [len(rows)]):
            lanes.append((col, rows[a:b]))
    return lanes


def forest_model(n, edges, seed, atomic_cas=True, max_lanes=3, lanes=None):
    """uint32 [n]: the labels after every lane of `edges` (or the given lanes [(col, rows)]) ran to its end under one random interleaving:
    pairs_labels_kernel's walk over the current values, `for (;;) { const uint32_t p = parent[x]; if (p >= x) break; x = p; }`"""
    rng = np.random.default_rng(seed)
    history = [[i] for i in range(n)]                 # every value parent[i] ever held; the last one is current
    running = []
    for col, rows in (lanes_of(edges, rng, max_lanes) if lanes is None else lanes):
        g = _lane(col, rows, atomic_cas)
        running.append([g, next(g)])
    steps = 0
    while running:
        k = int(rng.integers(0, len(running)))
        g, op = running[k]
        cell = history[op[1]]
        if op[0] == "load":
            result = cell[int(rng.integers(0, len(cell)))]
        elif op[0] == "load_now":
            result = cell[-1]
        elif op[0] == "cas":
            result = cell[-1]
            if result == op[2]:
                cell.append(op[3])
        elif op[0] == "min":
            result = cell[-1]
            if op[2] < result:
                cell.append(op[2])
        else:                                         # "store"
            result = None
            cell.append(op[2])
        steps += 1
        assert steps < 1000000, "the model does not end"
        try:
            running[k][1] = g.send(result)
        except StopIteration:
            running[k] = running[-1]
            running.pop()
    labels = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        x = i
        while history[x][-1] < x:
            x = history[x][-1]
        labels[i] = x
    return labels


def model_graph(kind, n, rng):
    """edges (a, b) of a small graph: "chain" (i, i + 1), "star0" / "starN" hub at 0 / n - 1, "clique", "sparse" random; chain and
    sparse under a random relabelling half of the time"""
    if kind == "chain":
        e = [(i, i + 1) for i in range(n - 1)]
    elif kind == "star0":
        e = [(0, i) for i in range(1, n)]
    elif kind == "starN":
        e = [(i, n - 1) for i in range(n - 1)]
    elif kind == "clique":
        m = min(n, 9)
        first = int(rng.integers(0, n - m + 1))
        e = [(a, b) for a in range(first, first + m) for b in range(a + 1, first + m)]
    elif kind == "sparse":
        k = int(rng.integers(n // 2, 2 * n))
        a, b = rng.integers(0, n, size=k), rng.integers(0, n, size=k)
        e = [(int(x), int(y)) for x, y in zip(a, b) if x != y]
    else:
        raise KeyError(kind)
    if kind in ("chain", "sparse") and rng.integers(0, 2):
        p = rng.permutation(n)
        e = [(int(p[a]), int(p[b])) for a, b in e]
    return [(min(a, b), max(a, b)) for a, b in e]


MODEL_KINDS = ("chain", "star0", "starN", "clique", "sparse")
LOST_HOOK_SEED = 0                                   # an interleaving under which the load-compare-store mutant loses a hook (test_the_model_sees_a_lost_hook)


# ------------------------------------------------------------------------------------------------------------------ B: stale bits
def dirty(planes, n_ref, nchar, how, seed=71):
    """a copy of exported tiles (uint8 [n_tiles, tile_bytes]) with, by a fixed-seed generator,
    "lanes": every lane at and past n_ref of the last tile overwritten;
    "bits":  in every lane of every tile the bits of the last alignment word at sites >= nchar and every word of the last group behind it;
    "both":  both.  Bits of sites below nchar in lanes below n_ref are never touched."""
    assert how in ("lanes", "bits", "both")
    W4 = ((nchar + 31) // 32 + 3) // 4
    out = planes.copy()
    t = out.reshape(-1).view(np.uint32).reshape(-1, W4, 4, 64, 4)                     # [tile, w4, plane, lane, j] as pack_tiles lays them out
    rng = np.random.default_rng(seed)
    if how in ("bits", "both"):
        keep = D.window_masks(W4 * 4, nchar, 0).reshape(W4, 1, 1, 4)                  # the bits of sites below nchar
        assert (keep.reshape(-1) != 0xFFFFFFFF).any(), "no padding to dirty at this length"
        noise = rng.integers(0, 2 ** 32, size=t.shape, dtype=np.uint64).astype(np.uint32)
        t[...] = (t & keep) | (noise & ~keep)
    if how in ("lanes", "both"):
        first = n_ref % 64
        assert first, "the last tile is full: no lane to dirty"
        t[-1, :, :, first:, :] = rng.integers(0, 2 ** 32, size=t[-1, :, :, first:, :].shape, dtype=np.uint64).astype(np.uint32)
    return out


# ------------------------------------------------------------------------------------------------------------------ C: the launch cut
LAUNCH_N, LAUNCH_NCHAR, LAUNCH_TRIM = 8200, 33, 1
LAUNCH_FAMILY = (5, 1023, 1024, 1025, 8191, 8192, 8199)       # a chain over the edges of the 1 024-row and 8 192-column launches


@functools.lru_cache(maxsize=None)
def launch_rows():
    """uint8 [8200, 33]: the database of test_links_across_launches -- random rows with N, R, Y and '-', a dense cluster inside the first
    launch's rows, and the seven-row chain family over both launch edges"""
    n, nchar = LAUNCH_N, LAUNCH_NCHAR
    rng = np.random.default_rng(23)
    rows = rng.choice(np.frombuffer(b"ACGTACGTACGTNRY-", dtype=np.uint8), size=(n, nchar))
    rows[1:1030:5] = rows[0]
    base = bytearray(np.random.default_rng(41).choice(_ACGT, size=nchar).tobytes())
    for k, pos in enumerate(LAUNCH_FAMILY):
        rows[pos] = np.frombuffer(bytes(base), dtype=np.uint8)
        base[2 + 4 * k] = b"ACGT"[(b"ACGT".index(base[2 + 4 * k]) + 1) % 4]
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def launch_seqs():
    return [r.tobytes() for r in launch_rows()]


@functools.lru_cache(maxsize=None)
def launch_counts(first, n):
    """pair_dist.plane_counts_of for rows [first, first + n) of launch_rows() against all columns at LAUNCH_TRIM, int32 [n, 8200, 5], read-only"""
    c = D.plane_counts_of(launch_seqs(), LAUNCH_NCHAR, trim=LAUNCH_TRIM, rows=(first, n))
    c.setflags(write=False)
    return c


def band_links(counts, first, metric, max_dist, min_compared=0, cols=None):
    """the (a, b), a < b, linked by the definition among rows [first, first + len(counts)) x cols (first, n) of a band of counters"""
    keep = K.linked(counts, metric, max_dist, min_compared)
    keep = keep & ((first + np.arange(counts.shape[0]))[:, None] < np.arange(counts.shape[1])[None, :])
    if cols is not None:
        keep[:, :cols[0]] = False
        keep[:, cols[0] + cols[1]:] = False
    pairs = np.argwhere(keep)
    pairs[:, 0] += first
    return pairs


_SET = np.zeros(256, dtype=np.uint8)                   # the set of bases behind every byte, bit 0 A .. bit 3 T: the planes of include/uvaia_gpu.h
for _ch, _s in zip(b"ACGTMRWSYKVHDB", (1, 2, 4, 8, 3, 5, 9, 6, 10, 12, 7, 11, 13, 14)):
    _SET[_ch] = _s
_MEET = np.array([[1.0 if a & b else 0.0 for b in range(16)] for a in range(16)], dtype=np.float32)


def uvaia_links_of_bytes(rows, trim, max_dist, min_compared=0, block=1024):
    """the (a, b), a < b, linked under the uvaia metric over [trim, nchar - trim) of a uint8 [n, nchar] array of upper-case text, by matrix
    products per block of rows as pair_link.snp_links_of_bytes does it: valid_pair_comparisons = V V' with V "the set is not empty",
    partial_matches = (X MEET) X' with X the one-hot code of the 16 sets and MEET[s][t] = the sets s and t intersect.  Sums of 0/1
    products below 2^24 in float32: exact.  (N, '-' and every other byte are the empty set; 'U' does not occur in these inputs.)"""
    w = _SET[rows[:, trim:rows.shape[1] - trim]]
    n, m = w.shape
    assert m < 2 ** 24
    onehot = (w[:, :, None] == np.arange(16, dtype=np.uint8)[None, None, :]).astype(np.float32)       # [n, site, set]
    meets = (onehot @ _MEET).reshape(n, -1)
    onehot = onehot.reshape(n, -1)
    valid = (w != 0).astype(np.float32)
    pairs = []
    for a in range(0, n, block):
        compared = valid[a:a + block] @ valid.T
        dist = compared - meets[a:a + block] @ onehot.T
        i, j = np.nonzero((dist <= max_dist) & (compared >= min_compared))
        i += a
        pairs.append(np.stack([i[i < j], j[i < j]], axis=1))
    return np.concatenate(pairs)


def launch_floor():
    """a floor that bites under uvaia at LAUNCH_TRIM: one more than the valid sites of row 0, whose copies then link no more (the family,
    ACGT at all 31 sites, still does)"""
    return int((_SET[launch_rows()[0, LAUNCH_TRIM:LAUNCH_NCHAR - LAUNCH_TRIM]] != 0).sum()) + 1


@functools.lru_cache(maxsize=None)
def launch_links(metric, max_dist, min_compared=0):
    """the links of all pairs of launch_rows() at LAUNCH_TRIM, int [k, 2], read-only (snp: the floor is not supported)"""
    if metric == "snp":
        assert min_compared == 0
        pairs = K.snp_links_of_bytes(launch_rows(), LAUNCH_TRIM, max_dist)
    else:
        pairs = uvaia_links_of_bytes(launch_rows(), LAUNCH_TRIM, max_dist, min_compared)
    pairs.setflags(write=False)
    return pairs


# ------------------------------------------------------------------------------------------------------------------ D: very short alignments
ShortQuery = collections.namedtuple("ShortQuery", "seqs consensus idx_c idx_m idx trim acgt")


def short_query(nchar):
    """a prepared query set to open an engine over at any length: the reference's preparation drops every query of fewer than 5 sites
    (`if (q->nchar < 5) continue;`, orc_query_keep_valid), so pair_dist.dummy_query has nothing to hand over at 1 and 2 sites.  One
    ACGT query as orc_query_create_indices leaves it: the consensus is the query, every site is common, none missing or polymorphic"""
    root = F.random_acgt(nchar, 3)
    return ShortQuery([root], root, np.arange(nchar, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0, False)
