"""Inputs that take the radius search (kernels_ball.inc, host_ball.inc, ensure_qgather in host_launch.inc) to its integer edges -- gathered
words that fill at exactly 32 bits and word groups that close at exactly four words, the switch to the hot column order at 512 polymorphic
columns, query tiles of 16 with a partial last one, the first query below the limit against a nearer later one, the early exit of the scan,
the comparisons of stage 1 on both sides of the radius, survivor lists around one tile of 64, ranges that start inside a tile -- and a small
model of the stage every reference takes (stage, gather_layout, running).  The model never judges a result: the oracle does.  Deterministic
and seeded; no GPU code here.  tests/test_ball_edges_cpu.py shows that every input reaches the edge it is built for,
tests/test_ball_edges_gpu.py runs the inputs on the device.

The edge table: which line each group is aimed at (kernels_ball.inc unless another file is named).
  A  columns gathered, their number    `if (__builtin_expect(++fill == 32, 0)) flush(o);`  `if (j == 3) {` of BitGather::flush (a group is written when
     and placement                     word ow & 3 == 3 closes)  `if (fill > 0) flush(o); while (ow < end_word) flush(o);` of finish  `hot.take(wd, mk[j], o);
                                       cold.take(wd, mk[4 + j], o);` (two walkers, one tile)  ensure_qgather: `if (n_idx >= 2 * BALL_HOT_COLS) {`,
                                       `c->ball.NH4 = n_hot / 128;`, `c->ball.NG4 = std::max(1, ...)`, the masks' `(col >> 7) * 8 + (i < n_hot ? 0 : 4) + ((col >> 5) & 3)`
                                       ball_gather_queries_kernel: `const int i = ow * 32 + b; if (i >= n_cols) break;`
  B  query tiles                       ball_scan_kernel: `uint32_t alive = q0 + QT <= nq ? ... : (1u << (nq - q0)) - 1u;`  `if (((alive >> q) & 1u) &&
                                       acc[q] < limit) key = ((unsigned long long)(unsigned)(q0 + q) << 32) | (unsigned)acc[q];`  `atomicMin(&first_key[k], key);`
                                       ball_finish2_kernel: `c + (key == ~0ull ? radius - c : (int)(unsigned)(key & 0xffffffffull))`
  C  the early exit                    ball_scan_kernel: `if (__builtin_amdgcn_ballot_w64(acc[q] < limit)) still |= 1u << q;`  `alive = still;`
                                       `for (int g = 0; g < NG4 && alive; g++)`  `const int limit = k < n ? radius - cdist[k] : 0;`  `if (k >= n) return;`
                                       ball_compact_kernel / ball_gather_cols_kernel: `const int r = k < n ? list[k] : list[n - 1];`
  D  stage 1's arithmetic              ball_stage1_kernel: `int md = min(dc, radius);`  `md += min(dm, radius);`  `if (2 * md >= radius) ask = true; else
                                       md = 2 * md;`  `if (has_c) {`  `if (has_m) {`
  E  the survivor list, buffers        ball_stage1_kernel: `const int k = atomicAdd(n_survivors, 1); survivors[k] = r; cdist[k] = md;`  host_ball.inc:
     reused                            `const int mt = (n_ask + 63) / 64;`  `if (c->ball.d_key.cap < (size_t)mt * 64) {`  `hipMemsetAsync(c->ball.d_key, 0xFF,
                                       (size_t)mt * 64 * ...)`  `b->reserve(c, cap)` of the three result arrays  `if (fused && c->ball.d_ga.reserve(c, (size_t)n_tiles * tile_u4))`
  F  ranges and batch sizes            ball_stage1_kernel: `if (r < r_lo || r >= r_hi) return;`  `mindist[r - r_lo] = md;`  ball_finish2_kernel:
                                       `mindist[list[k] - r_lo]`  host_ball.inc: the arguments of ball_range in uvaia_gpu_ball_resident, `if (first + n >
                                       c->db_n)`, `if ((size_t)n_ref > c->max_pool)` of uvaia_gpu_ball and uvaia_gpu_ball_packed"""
import collections
import functools

import numpy as np

import fixtures as F
import oracle_lib as O

# ---- copies of the code's constants; each moves with the line it mirrors
QTB = 16                    # `constexpr int QTB = 16;`  queries of one wave of ball_scan_kernel (ball_range, host_ball.inc)
BALL_HOT_COLS = 256         # `constexpr int BALL_HOT_COLS = 256;`  (ensure_qgather, host_launch.inc)
GROUP_COLS = 128            # `c->ball.NG4 = std::max(1, c->ball.NH4 + (n_idx - n_hot + 127) / 128);`  columns of a word group (a uint4 of 32-column words)
WORD_COLS = 32              # `if (__builtin_expect(++fill == 32, 0)) flush(o);`  (BitGather::take, kernels_ball.inc)
TILE = 64                   # `const int k = blockIdx.x * 64 + lane;`  references of a tile (ball_compact_kernel, ball_gather_cols_kernel)
TILES_PER_BLOCK = 4         # `const int trel = blockIdx.x * 4 + wave;`  (ball_stage1_kernel); `const int tile = grp * 4 + wave;` (ball_scan_kernel)

MAX_POOL = 512              # what the device tests open every engine with
INVALID = b"NnXx-?Oo."      # `const char *inv  = "NnXx-?Oo.";` (oracle/uvaia_oracle.c): never counted, in either mode

_NEXT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    _NEXT[_a] = _b
_USABLE = {False: np.ones(256, dtype=bool), True: np.zeros(256, dtype=bool)}
_USABLE[False][list(INVALID)] = False           # default mode: both valid and the text differs (orc_dist_text_indelcheck)
_USABLE[True][list(b"ACGTacgt")] = True         # --acgt: both ACGT and different (orc_dist_acgt)


def rot(a, k=1):
    """every A, C, G, T moved k letters on (A -> C -> G -> T -> A); other bytes stay"""
    a = np.asarray(a, dtype=np.uint8)
    for _ in range(k):
        a = _NEXT[a]
    return a


def arr(seq):
    return np.frombuffer(seq, dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------------------------ query sets
QSet = collections.namedtuple("QSet", "name nchar root seqs names n_idx n_idx_m")


def make_qset(name, nchar, seed, differ, n_at=None):
    """a random ACGT root and one query per entry of differ: the root with the next letter at those columns and N at the columns of n_at.
    n_idx / n_idx_m: the polymorphic columns and the constant columns with a missing query that the oracle must find (the CPU test asks it)"""
    root = arr(F.random_acgt(nchar, seed))
    nq = len(differ)
    n_at = n_at or [[] for _ in range(nq)]
    seqs = []
    for cols, ns in zip(differ, n_at):
        s = root.copy()
        cols = np.asarray(cols, dtype=np.int64)
        s[cols] = rot(root[cols])
        s[np.asarray(ns, dtype=np.int64)] = ord("N")
        seqs.append(s.tobytes())
    poly = set(c for cols in differ for c in cols) if nq > 1 else set()
    # a column where every query differs from the root is constant again
    poly = set(c for c in poly if sum(c in set(cols) for cols in differ) < nq)
    miss = set(c for ns in n_at for c in ns) if nq > 1 else set()
    assert not (poly & miss)
    return QSet(name, nchar, root, tuple(seqs), tuple("q%d" % i for i in range(nq)), len(poly), len(miss))


@functools.lru_cache(maxsize=None)
def _prepared(key, acgt, dist):
    qs = QSETS[key]()
    return O.Query(list(qs.seqs), list(qs.names), dist=dist, acgt=acgt, is_ball=True)


def prepared(key, acgt, radius):
    """the oracle's prepared query structure of query set `key` for a search of that radius (cq->dist = radius - 1)"""
    return _prepared(key, bool(acgt), radius - 1)


QSETS = {}                  # key -> builder of the QSet (filled by the groups below)


def qset(key):
    return QSETS[key]()


# ------------------------------------------------------------------------------------------------------------------ the model
Model = collections.namedtuple("Model", "acgt cons idx_c idx_m idx qs usable root_idx")


def model_of(q):
    m = getattr(q, "_ball_edges_model", None)
    if m is None:
        qs, usable = np.stack([arr(s) for s in q.seqs]), _USABLE[bool(q.acgt)]
        root_idx = np.array([np.bincount(qs[:, c][usable[qs[:, c]]]).argmax() for c in q.idx], dtype=np.uint8)   # the letter most queries hold
        m = Model(q.acgt, arr(q.consensus), q.idx_c, q.idx_m, q.idx, qs, usable, root_idx)
        q._ball_edges_model = m
    return m


def _dist(m, a, b, cols):
    """ball_one's `dist` without its stop: columns where both are usable in this mode and the bytes differ (b: one row or several)"""
    a, b = a[cols], b[..., cols]
    return ((a != b) & m.usable[a] & m.usable[b]).sum(axis=-1)


Stage = collections.namedtuple("Stage", "dc dm md asks first_query d_first")


def stage(q, ref, radius):
    """(dc, dm, md_after_consensus, asks, first_query, d_first) of one reference, after ball_one (oracle/uvaia_oracle.c):
        dist (seq, q->consensus, n_idx_c, radius, min_dist, q->idx_c);   if (*min_dist >= radius) return;
        dist (seq, q->consensus, n_idx_m, radius, min_dist, q->idx_m);   *min_dist += c_dist;   if (*min_dist >= radius) return;
        for (i = 0; i < q->ntax && (*min_dist + c_dist) >= radius; i++) dist (seq, q->seq[i], n_idx, radius - c_dist, min_dist, q->idx);
    dc, dm: the whole counts on idx_c and idx_m; md: min(dc, radius), plus min(dm, radius) where that was below the radius; asks: the loop
    over the queries runs (md < radius <= 2 md); first_query, d_first: the first query in prepared order whose distance on idx is below
    radius - md, and that distance (None, None where there is none or the loop does not run)"""
    m = model_of(q)
    r = arr(ref) if isinstance(ref, (bytes, bytearray)) else ref
    dc, dm = int(_dist(m, r, m.cons, m.idx_c)), int(_dist(m, r, m.cons, m.idx_m))
    md = min(dc, radius)
    if md < radius:
        md += min(dm, radius)
    asks = md < radius and 2 * md >= radius
    first, d_first = None, None
    if asks:
        d = _dist(m, r, m.qs, m.idx)
        below = np.nonzero(d < radius - md)[0]
        if len(below):
            first, d_first = int(below[0]), int(d[below[0]])
    return Stage(dc, dm, md, asks, first, d_first)


def branch(st, radius):
    """which way out of ball_one a reference takes"""
    if st.dc >= radius:
        return "first"                          # `if (*min_dist >= radius) return;` after idx_c
    if st.md >= radius:
        return "second"                         # ... after idx_m
    return "loop" if st.asks else "doubled"     # the loop's condition holds on entry | *min_dist += c_dist without a pass


def answer(st, radius):
    """what the model expects in cq->mindist (the CPU test holds it against the oracle: it checks the model, never the engine)"""
    if st.md >= radius or not st.asks:
        return st.md if st.md >= radius else 2 * st.md
    return st.md + (st.d_first if st.first_query is not None else radius - st.md)


def n_asked(q, refs, radius):
    return sum(stage(q, r, radius).asks for r in refs)


Layout = collections.namedtuple("Layout", "order n_hot NH4 NG4 score")


def gather_layout(q):
    """ensure_qgather's order of the columns of query->idx in the gathered words: below 2 * BALL_HOT_COLS the column order; from there on
    the BALL_HOT_COLS columns with the most queries off the column's most frequent character first (ties: the lower column), then the
    others, each set in increasing column order.  score: ball_column_diversity_kernel's count per column of idx"""
    m = model_of(q)
    n_idx = len(m.idx)
    cols = m.qs[:, m.idx] if n_idx else np.zeros((len(m.qs), 0), dtype=np.uint8)
    ok = m.usable[cols]
    score = np.zeros(n_idx, dtype=np.int64)
    for i in range(n_idx):
        c = cols[ok[:, i], i]
        score[i] = len(c) - (np.bincount(c).max() if len(c) else 0)
    n_hot = 0
    order = np.asarray(m.idx, dtype=np.int64)
    if n_idx >= 2 * BALL_HOT_COLS:                                  # `if (n_idx >= 2 * BALL_HOT_COLS) {`
        n_hot = BALL_HOT_COLS
        by_score = np.argsort(-score, kind="stable")                # `std::stable_sort(... score[a] > score[b])`
        is_hot = np.zeros(n_idx, dtype=bool)
        is_hot[by_score[:n_hot]] = True
        order = np.concatenate([order[is_hot], order[~is_hot]])
    NH4 = n_hot // GROUP_COLS                                       # `c->ball.NH4 = n_hot / 128;`
    NG4 = max(1, NH4 + (n_idx - n_hot + GROUP_COLS - 1) // GROUP_COLS)
    return Layout(order, n_hot, NH4, NG4, score)


def running(q, ref):
    """int [query, word group]: a reference's count against every query after each word group of the gathered order (ball_scan_kernel's acc)"""
    m, lay = model_of(q), gather_layout(q)
    r = arr(ref) if isinstance(ref, (bytes, bytearray)) else ref
    out = np.zeros((len(m.qs), lay.NG4), dtype=np.int64)
    for g in range(lay.NG4):
        cols = lay.order[g * GROUP_COLS:(g + 1) * GROUP_COLS]
        out[:, g] = _dist(m, r, m.qs, cols) if len(cols) else 0
    return np.cumsum(out, axis=1)


# ------------------------------------------------------------------------------------------------------------- reference builders
IUPAC_AT_IDX = b"RYN-RKM-N"


def toward_consensus_distance(m, r, dc, dm, rng):
    """r with dc columns of idx_c and dm columns of idx_m moved off the consensus (dc < 0: all of idx_c); what a set lacks goes to the other"""
    if dc < 0:
        dc = len(m.idx_c) if len(m.idx_c) else len(m.idx_m)
    if dc > len(m.idx_c):
        dc, dm = len(m.idx_c), dm + dc - len(m.idx_c)
    if dm > len(m.idx_m):
        dc, dm = min(len(m.idx_c), dc + dm - len(m.idx_m)), len(m.idx_m)
    for cols, k in ((m.idx_c, dc), (m.idx_m, dm)):
        if k:
            at = rng.choice(cols, size=k, replace=False)
            r[at] = rot(m.cons[at])
    return r


def on_idx(m, i, rng, iupac):
    """the root or a query, up to six columns of idx moved to another letter, and now and then an ambiguity code, an N or a gap there:
    R against A is one difference in default mode and none with --acgt, R against R none, N and - never count"""
    base = m.cons.copy()
    if len(m.idx) == 0:
        return base
    if i % 3:
        base[m.idx] = m.qs[i % len(m.qs)][m.idx]
    else:                                                           # the root on idx
        base[m.idx] = m.root_idx
    k = min(int(rng.integers(0, 7)), len(m.idx))
    if k:
        at = rng.choice(m.idx, size=k, replace=False)
        base[at] = rot(base[at], int(rng.integers(1, 4)))
    if iupac and i % 4 == 1:
        at = rng.choice(m.idx, size=min(2, len(m.idx)), replace=False)
        base[at] = np.frombuffer(IUPAC_AT_IDX, dtype=np.uint8)[rng.integers(0, len(IUPAC_AT_IDX), size=len(at))]
    return base


def mutant_refs(q, n, seed, md_of, iupac=True):
    """n references: on_idx() with md_of(i) columns of the constant sets moved off the consensus, split at random between idx_c and idx_m"""
    m, rng, out = model_of(q), np.random.default_rng(seed), []
    for i in range(n):
        r = on_idx(m, i, rng, iupac)
        md = md_of(i)
        dm = int(rng.integers(0, md + 1)) if len(m.idx_m) else 0
        out.append(toward_consensus_distance(m, r, md - dm, dm, rng).tobytes())
    return out


# ------------------------------------------------------------------------------------- A: number and placement of gathered columns
A_RADIUS = 6
A_NREF = 130
A_N_IDX = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 640)
A_NQ = {0: 1, 1: 2, 31: 16, 32: 16, 33: 16, 127: 5, 128: 5, 129: 2, 255: 17, 256: 17, 257: 17, 511: 33, 512: 33, 513: 17, 640: 17}
A_N_IDX_M = {0: 0, 1: 3, 129: 0, 512: 7, 513: 40}                      # 12 elsewhere
A_PACKED_FROM = 64                                                  # a 32-column word's first column

ACase = collections.namedtuple("ACase", "name nchar n_idx placement nq n_idx_m")


def _a_cases():
    out = []
    for n in A_N_IDX:
        places = ("spread", "packed") if n < 2 * BALL_HOT_COLS else ("spread-hot", "hot-above", "hot-interleaved")
        if n == 0:
            places = ("spread",)
        for p in places:
            out.append(ACase("n%d-%s" % (n, p), 2000, n, p, A_NQ[n], A_N_IDX_M.get(n, 12)))
    for n in (33, 129, 513):
        out.append(ACase("n%d-ends" % n, 2000, n, "ends", A_NQ[n], A_N_IDX_M.get(n, 12)))
    for n in (1, 32, 33):
        out.append(ACase("n%d-last-group" % n, 2000, n, "last-group", A_NQ[n], A_N_IDX_M.get(n, 12)))
    out.append(ACase("sites129-n33", 129, 33, "ends", 16, 5))          # W4 = 2, the second word group holds one site, and it is gathered
    out.append(ACase("sites100-n0", 100, 0, "spread", 1, 0))           # W4 = 1, nothing gathered
    out.append(ACase("sites100-n20", 100, 20, "ends", 4, 3))
    return out


A_CASES = _a_cases()
A_NAMES = [c.name for c in A_CASES]


def a_columns(case):
    """(the designated columns in increasing order, those of them meant to be hot)"""
    n, nchar = case.n_idx, case.nchar
    hot = np.zeros(0, dtype=np.int64)
    if case.placement == "spread":
        cols = (2 * np.arange(n) + 1) * nchar // (2 * n) if n else np.zeros(0, dtype=np.int64)
    elif case.placement == "ends":                                  # column 0 and column nchar - 1 are among them
        cols = np.arange(n) * (nchar - 1) // (n - 1)
        hot = cols[0:2 * BALL_HOT_COLS:2] if n >= 2 * BALL_HOT_COLS else hot
    elif case.placement == "packed":                                # whole 32-column words: masks of 0xffffffff, a gathered word fills at a source word's end
        cols = A_PACKED_FROM + np.arange(n)
    elif case.placement == "last-group":                            # all inside word group W4 - 1
        first = (nchar - 1) // GROUP_COLS * GROUP_COLS
        cols = first + np.arange(n) * (nchar - first) // n
    elif case.placement == "spread-hot":                            # every other one of the first 512 is hot
        cols = (2 * np.arange(n) + 1) * nchar // (2 * n)
        hot = cols[0:2 * BALL_HOT_COLS:2]
    elif case.placement == "hot-above":                             # the hot columns all above the cold ones
        cols = A_PACKED_FROM + np.arange(n)
        hot = cols[n - BALL_HOT_COLS:]
    elif case.placement == "hot-interleaved":                       # word by word: hot, cold, hot, cold ... for eight words each, the rest cold
        cols = A_PACKED_FROM + np.arange(n)
        word = np.arange(n) // WORD_COLS
        hot = cols[(word % 2 == 0) & (word < 2 * BALL_HOT_COLS // WORD_COLS)]
    cols = np.asarray(cols, dtype=np.int64)
    assert len(np.unique(cols)) == n and (n == 0 or (cols[0] >= 0 and cols[-1] < nchar))
    assert len(hot) == (BALL_HOT_COLS if n >= 2 * BALL_HOT_COLS else 0)
    return cols, hot


def columns_to_queries(cols, hot, nq, n_idx_m, nchar):
    """differ / n_at of make_qset: a cold column has one query off the root, a hot one half of them; the N columns are constant ones"""
    hot_set = set(int(c) for c in hot)
    differ = [[] for _ in range(nq)]
    for k, c in enumerate(int(c) for c in cols):
        owners = [(k + j) % nq for j in range(nq // 2)] if c in hot_set else [k % nq]
        for o in owners:
            differ[o].append(c)
    free = [c for c in range(nchar) if c not in set(int(x) for x in cols)]
    n_at = [[] for _ in range(nq)]
    for j in range(n_idx_m):
        n_at[j % nq].append(free[(j * 37 + 5) % len(free)] if len(free) > 37 * n_idx_m else free[j])
    assert len(set(c for ns in n_at for c in ns)) == n_idx_m
    return differ, n_at


def _a_qset(case):
    cols, hot = a_columns(case)
    differ, n_at = columns_to_queries(cols, hot, case.nq, case.n_idx_m, case.nchar)
    return make_qset("A-" + case.name, case.nchar, 20270100 + A_NAMES.index(case.name), differ, n_at)


for _c in A_CASES:
    QSETS["A-" + _c.name] = functools.lru_cache(maxsize=None)(functools.partial(_a_qset, _c))


def a_md(i):
    """most references go on to the queries at radius 6 (3, 4, 5); one in sixteen stops at the consensus, one takes the doubled distance"""
    return (3, 4, 5, 3, 4, 5, 3, 4, 5, 0, 4, 3, 5, 6, 3, 4)[i % 16]


@functools.lru_cache(maxsize=None)
def group_a(name, acgt):
    """(prepared query, references) of one case"""
    q = prepared("A-" + name, acgt, A_RADIUS)
    return q, mutant_refs(q, A_NREF, 20270200 + A_NAMES.index(name), a_md)


def a_expected_layout(case):
    """(NH4, NG4) as the issue states them"""
    n_hot = BALL_HOT_COLS if case.n_idx >= 2 * BALL_HOT_COLS else 0
    nh4 = n_hot // GROUP_COLS
    return nh4, max(1, nh4 + -(-(case.n_idx - n_hot) // GROUP_COLS))


# --------------------------------------------------------------------------------------------------------------- B: query tiles
B_RADIUS = 8
B_NQ = (1, 2, 15, 16, 17, 31, 32, 33)
B_POOL = np.arange(10, 30)                                          # constant columns that carry a reference's distance to the consensus


def _b_qset(nq):
    """query i: two own columns off the root, and 0, 1 or 2 N at constant columns of its own, so that preparation reorders the set"""
    differ = [[40 + 50 * i, 57 + 50 * i] for i in range(nq)]
    n_at = [[45 + 50 * i + j for j in range((i * 7) % 3)] if nq > 1 else [] for i in range(nq)]
    return make_qset("B-%d" % nq, 2000, 20270300 + nq, differ, n_at)


for _n in B_NQ:
    QSETS["B-%d" % _n] = functools.lru_cache(maxsize=None)(functools.partial(_b_qset, _n))

BRef = collections.namedtuple("BRef", "name ref first_query d_first")


def b_positions(nq):
    """0, 15, 16, nq - 1 and the last position of a full tile of 16, where the set has them"""
    return sorted(p for p in {0, QTB - 1, QTB, nq - 1, nq // QTB * QTB - 1} if 0 <= p < nq)


@functools.lru_cache(maxsize=None)
def group_b(nq, acgt):
    """(prepared query, [BRef]).  With two own columns per query a reference equal to one query is at 4 from every other, the root at 2
    from all; an N at one of a query's own columns takes that column out of every count."""
    q = prepared("B-%d" % nq, acgt, B_RADIUS)
    m = model_of(q)
    root = qset("B-%d" % nq).root if nq > 1 else m.cons         # (one query: it is the consensus, and every column is constant)
    own = [np.nonzero((m.qs[p] != root) & (m.qs[p] != ord("N")))[0] for p in range(len(m.qs))]

    def ref(c, equal=(), n_at_own=()):
        r = root.copy()
        for p in equal:
            r[own[p]] = m.qs[p][own[p]]
        for p in n_at_own:
            r[own[p][0]] = ord("N")
        r[B_POOL[:c]] = rot(root[B_POOL[:c]])
        return r.tobytes()

    out = []
    if nq == 1:                                                     # no polymorphic column: every distance on idx is 0
        return q, [BRef("one-query-c%d" % c, ref(c), 0, 0) for c in (4, 7)]
    for p in b_positions(nq):
        # limit 4: the query at p is at 0, every other one at exactly 4 = the limit, which must not end the walk
        out.append(BRef("only-%d-at-0" % p, ref(4, equal=(p,)), p, 0))
        # limit 2: the query at p is at 1 = limit - 1, every other one at 2
        out.append(BRef("only-%d-at-limit-1" % p, ref(6, n_at_own=(p,)), p, 1))
    out.append(BRef("none-below", ref(6), None, None))             # limit 2, every query at 2: the answer is the radius
    out.append(BRef("all-below", ref(5), 0, 2))                     # limit 3: the first one it is
    for early, late in ((3, 20), (3, 9), (15, 16), (0, nq - 1)):    # two tiles | one tile | neighbours across the tile edge | the ends
        if early < late < nq:
            # limit 4: the query at `early` is at 3 = limit - 1, the one at `late` at 0, every other at 4: the first one below the
            # limit answers, c + 3, and a kernel that takes the nearest gives c + 0
            out.append(BRef("first-%d-not-nearest-%d" % (early, late), ref(4, equal=(late,), n_at_own=(early,)), early, 3))
    return q, out


# ------------------------------------------------------------------------------------------------------------ C: the early exit
C_RADIUS = 10
C_DC, C_DM = 3, 2                                                   # every reference of the group: c_dist 5, limit 5
C_LIMIT = C_RADIUS - C_DC - C_DM
C_NQ = 17
C_LANE, C_QUERY = 37, 2                                             # stays below its limit against query 2 through the last word group
C_LANE2, C_QUERY2 = 11, 9                                           # stays below against query 9 through group 0, passes it in group 1
C_CASES = {"cold511": 511, "hot640": 640}                           # column order, 4 word groups | hot order, 2 + 3 word groups


def _c_qset(name):
    n = C_CASES[name]
    cols = (2 * np.arange(n) + 1) * 2000 // (2 * n)
    hot = cols[0:2 * BALL_HOT_COLS:2] if n >= 2 * BALL_HOT_COLS else cols[:0]
    differ, n_at = columns_to_queries(cols, hot, C_NQ, 6, 2000)
    return make_qset("C-" + name, 2000, 20270400 + n, differ, n_at)


for _k in C_CASES:
    QSETS["C-" + _k] = functools.lru_cache(maxsize=None)(functools.partial(_c_qset, _k))


@functools.lru_cache(maxsize=None)
def group_c(name, acgt):
    """(prepared query, 65 references that all go on to the queries).  An ordinary lane holds a third letter -- neither the root's nor any
    query's -- at `limit` or more columns of word group 0, so it is at its limit against every query after that group.  Lane 37 is query
    2 with a third letter at limit - 1 columns of the later groups, one of them in the last; lane 11 is query 9 with `limit` of them in
    group 1.  references[:64] is the one-tile case, all 65 the case with one real lane in the second gathered tile."""
    q = prepared("C-" + name, acgt, C_RADIUS)
    m, lay = model_of(q), gather_layout(q)
    root = qset("C-" + name).root
    rng = np.random.default_rng(20270450 + C_CASES[name])
    groups = [lay.order[g * GROUP_COLS:(g + 1) * GROUP_COLS] for g in range(lay.NG4)]
    refs = []
    for i in range(TILE + 1):
        r = m.cons.copy()
        if i == C_LANE:
            r[m.idx] = m.qs[C_QUERY][m.idx]
            at = [groups[lay.NG4 - 1 - j % (lay.NG4 - 1)][5 + 17 * j] for j in range(C_LIMIT - 1)]
        elif i == C_LANE2:
            r[m.idx] = m.qs[C_QUERY2][m.idx]
            at = groups[1][3:3 + 11 * C_LIMIT:11]
        else:
            r[m.idx] = m.qs[i % C_NQ][m.idx] if i % 4 else root[m.idx]
            at = rng.choice(groups[0], size=C_LIMIT + i % 3, replace=False)
        at = np.asarray(at, dtype=np.int64)
        r[at] = rot(root[at], 2)
        refs.append(toward_consensus_distance(m, r, C_DC, C_DM, rng).tobytes())
    return q, refs


# ---------------------------------------------------------------------------------------------------------- D: stage 1 arithmetic
D_RADII = (1, 2, 3, 10, 11)
D_NREF = 120
D_SETS = ("main", "no-idx-m", "no-idx-c", "all-polymorphic")
D_EXPECT = {"main": (2000 - 60 - 30, 30, 60), "no-idx-m": (2000 - 60, 0, 60), "no-idx-c": (0, 184, 16), "all-polymorphic": (0, 0, 130)}   # idx_c, idx_m, idx


def _d_qset(name):
    if name in ("main", "no-idx-m"):
        cols = (2 * np.arange(60) + 1) * 2000 // 120
        differ, n_at = columns_to_queries(cols, cols[:0], 12, 30 if name == "main" else 0, 2000)
        return make_qset("D-" + name, 2000, 20270500, differ, n_at)
    if name == "no-idx-c":                                           # 200 sites, 8 queries: two own columns each, every other column has one query with N
        differ = [[12 * i + 3, 12 * i + 100] for i in range(8)]
        poly = set(c for d in differ for c in d)
        n_at = [[] for _ in range(8)]
        for j, c in enumerate(c for c in range(200) if c not in poly):
            n_at[j % 8].append(c)
        return make_qset("D-" + name, 200, 20270501, differ, n_at)
    differ = [list(range(i, 130, 8)) for i in range(8)]              # 130 sites, every column polymorphic
    return make_qset("D-" + name, 130, 20270502, differ)


for _k in D_SETS:
    QSETS["D-" + _k] = functools.lru_cache(maxsize=None)(functools.partial(_d_qset, _k))


def d_recipes(radius):
    """(dc, dm) pairs on both sides of every comparison of stage 1 (dc < 0: all of idx_c)"""
    R = radius
    out = [(R - 1, 0), (R, 0), (R + 1, 0), (-1, 0)]                                     # `int md = min(dc, radius);` `if (md < radius)`
    for s in (R - 1, R, R + 1):                                                         # `md += min(dm, radius);` `if (md < radius)`
        out += [(s // 2, s - s // 2), (0, s), (max(s - 1, 0), min(s, 1))]
    out += [(0, R + 1), (0, R + 2), (1, R + 3), (R - 1, R + 2)]                         # dm alone above the radius
    for t in (R - 1, R, R + 1):                                                         # `if (2 * md >= radius) ask = true; else md = 2 * md;`
        if t % 2 == 0:
            out += [(t // 2, 0), (0, t // 2), (t // 4, t // 2 - t // 4)]
    out += [(0, 0), (0, 0)]                                                             # md = 0
    return [(dc, dm) for dc, dm in out if dc >= -1 and dm >= 0]


@functools.lru_cache(maxsize=None)
def group_d(name, acgt, radius, n=D_NREF):
    """(prepared query, n references): the recipes in turn, each on another root-or-query of on_idx(); a longer list repeats the recipes
    on further ones and starts with the shorter list"""
    q = prepared("D-" + name, acgt, radius)
    m, rng, refs = model_of(q), np.random.default_rng(20270550 + radius), []
    rec = d_recipes(radius)
    for i in range(n):
        dc, dm = rec[i % len(rec)]
        r = on_idx(m, i + i // len(rec), rng, True)
        refs.append(toward_consensus_distance(m, r, dc, dm, rng).tobytes())
    return q, refs


# ------------------------------------------------------------------------------- E: length of the survivor list, buffers reused
E_RADIUS = 6
E_NREF = 1400
E_COUNTS = (0, 1, 63, 64, 65, 256, 257)
E_ORDER = (257, 1, 64, 0, 65, 63, 256)                              # a short list follows a long one in the same key and tile buffers
E_SUBSET = 400
E_FIRST_APPEND = 70


def _e_qset():
    cols = (2 * np.arange(300) + 1) * 2000 // 600
    differ, n_at = columns_to_queries(cols, cols[:0], 17, 20, 2000)
    return make_qset("E", 2000, 20270600, differ, n_at)


QSETS["E"] = functools.lru_cache(maxsize=None)(_e_qset)


def e_md(i):
    """every second reference goes on to the queries"""
    return (3, 0, 4, 6, 5, 2, 3, 9, 4, 1, 5, 7)[i % 12]


@functools.lru_cache(maxsize=None)
def group_e(acgt):
    """(prepared query, 1 400 references, bool per reference: the model says it goes on to the queries)"""
    q = prepared("E", acgt, E_RADIUS)
    refs = mutant_refs(q, E_NREF, 20270650, e_md)
    return q, refs, np.array([stage(q, r, E_RADIUS).asks for r in refs])


def e_subset(asks, count, layout):
    """indices of E_SUBSET references of which exactly `count` go on: "scattered" over all tiles of the subset, or in "one-tile", from
    the second tile's first lane on (64 fit in it; a longer list runs on into the next tiles)"""
    yes, no = list(np.nonzero(asks)[0]), list(np.nonzero(~asks)[0])
    if layout == "scattered":
        at = set((j * E_SUBSET) // count for j in range(count))
    else:
        at = set(range(TILE, TILE + count))
    assert len(at) == count
    out = [yes.pop(0) if k in at else no.pop(0) for k in range(E_SUBSET)]
    return [int(x) for x in out]


# ------------------------------------------------------------------------------------------------------ F: ranges and batch sizes
F_RADIUS = 10
F_DB = 200                                                          # three tiles and 8 lanes
F_RANGES = ((0, 200), (0, 1), (63, 1), (63, 2), (64, 64), (65, 63), (1, 198), (128, 72), (199, 1), (100, 0))
F_BATCHES = (1, 63, 64, 65, 512)


def group_f(acgt):
    """(prepared query, 512 references: group D's of radius 10 and their continuation; the first 200 are the resident database)"""
    return group_d("main", acgt, F_RADIUS, MAX_POOL)
