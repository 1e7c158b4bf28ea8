"""Inputs that take the slice plan of the resident search (host_resident.inc: plan_subslices, consumed by run_subslices and uvaia_gpu_db_rederive) to its
branch points -- the quarter rule with a 70 % first slice, the head / middle / tail layout with and without the 131 072 slice before the tail, pools
that are cut again, a pool that is ignored, the 70 % first slice at 63 query tiles -- and a restatement of the planner (plan) that says where each
input's slices begin.  The restatement never judges a result: the oracle does, and tests/test_slice_edges_gpu.py holds it against
uvaia_gpu_search_plan before it uses a boundary.  Deterministic and seeded; no GPU code here.  tests/test_slice_edges_cpu.py shows with the oracle
alone that every input does what it is built for.

The references of a case come closer to the queries along the stream: a staircase of deficits (sites that are N or differ from the root), one step
every few thousand references.  A reference on its step carries HIGH substitutions, except the first two of every step, which carry LOW ones (both
numbers are staircases of their own, falling along the stream); all the others are noise, worse than their step by four deficits and more, with
at least HIGH substitutions and the letters of a random query at the queries' own columns.  The gate admits nothing with more mismatches than the worst
kept entry has, so whatever enters under a low tolerance keeps a successor in the heap for good: the two low references of a step are the worst of
their step and end up worst kept (the tolerance falls); the next step's low ones replace them, an entry of HIGH substitutions becomes the worst (the
tolerance rises) and lets the step's other references in.  A snapshot taken while the tolerance is low cuts the pre-score of every reference of HIGH
substitutions short, which is what makes a pool boundary matter (case e).  So every step brings admissions, and a slice that is dropped, scanned
twice, replayed out of order or behind the wrong snapshot changes the entered flags.  At the last position of every slice and the first of the next
sits a pair of identical references better than the whole staircase: both stay in the final heaps and only the ordinal tells them apart."""
import collections
import functools

import numpy as np

import oracle_lib as O

# ---- copies of the code's constants; each moves with the line it mirrors (host_resident.inc unless another file is named)
SUBSLICE = 25088             # `size_t subslice = 25088;` (host_ctx.inc)
HALF_NQT = 32                # `if (nqt <= 32) sub /= 2;`
FULL_NQT = 63                # `if (nqt < 63) sub = std::min(pool, (sub * 63 / (size_t)std::max(nqt, 1) + 63) / 64 * 64);`
QUARTER_NQT = 4              # `if (nqt < 4) sub = std::min(pool, std::max<size_t>(65536, ((pool + 3) / 4 + 63) / 64 * 64));`
QUARTER_MIN = 65536          # the same line: no slice of the four below this
HEAD_TAIL_NQT = 17           # `#define HEAD_TAIL_NQT 17`
HEAD_TAIL_POOL = 8 * 65536   # `if (nqt < HEAD_TAIL_NQT && !c->subslice_forced && pe - a >= 8 * 65536) {`
HEAD = TAIL = 65536          # `const size_t head = 65536, tail = 65536, pre = (nqt < 4 && pe - a >= 12 * 65536) ? 131072 : 0, ...`
PRE = 131072                 # the same line
PRE_POOL = 12 * 65536        # the same line
PRE_NQT = 4                  # the same line
FIRST_PCT = 70               # `const int first_pct = c->first_slice_pct >= 0 ? c->first_slice_pct : ((lean_replay_context(c) && c->replay_lq == 0) ? 0 : 70);`
FIRST_MIN_SLICES = 3         # `if (first_pct > 0 && first_pct < 100 && ns >= 3 && !c->subslice_forced) {`
LEAN_NQ = 256                # `if (c->replay_lq < 0) c->replay_lq = (nq < 256) ? 1 : 0;` (host_qprep.inc)
LEAN_NBEST = 127             # `... && c->n_idx_c == 0 && c->k <= 127; }` of lean_replay_context (host_launch.inc)
PACKED_NQ = 32               # `c->scan_variant = ... : (c->nq <= 32 ? 0 : 2);` (host_open.inc)
NBUF = 4                     # `constexpr int NBUF = 4;` (uvaia_gpu.hip)
TILE = 64

WINDOW = 8192                # every window of this many stream positions holds an admission
NCHAR = 128
NBEST = 24                   # two slots for every pair at a slice boundary (at most eight boundaries) and eight that turn over


def _r64(x):
    return (x + 63) // 64 * 64


def plan(first, n, pool, nq, n_idx_c, acgt, nbest=NBEST, subslice_refs=0, first_pct=None, active=None, packed=None):
    """plan_subslices restated: [(first, length, opens a pool)].  nq queries (active = (q0, q1) narrows them), first_pct None = the library's choice;
    packed None = the library's choice of scan by the number of queries (what use_ext, and through it lean_replay_context, depends on)."""
    q0, q1 = active or (0, nq)
    nqt = (q1 + 15) // 16 - q0 // 16
    forced = subslice_refs > 0
    if n_idx_c == 0:
        pool = max(n, 1)
    sub = subslice_refs if forced else SUBSLICE
    if nqt <= HALF_NQT:
        sub //= 2
    if nqt < FULL_NQT:
        sub = min(pool, _r64(sub * 63 // max(nqt, 1)))
    if nqt < QUARTER_NQT:
        sub = min(pool, max(QUARTER_MIN, _r64((pool + 3) // 4)))
    if forced:
        sub = min(pool, subslice_refs)
    if first_pct is None:
        packed = (nq <= PACKED_NQ) if packed is None else packed
        use_ext = (not acgt) and packed
        lean = (not use_ext) and (not acgt) and n_idx_c == 0 and max(2, nbest) <= LEAN_NBEST and nq >= LEAN_NQ
        first_pct = 0 if lean else FIRST_PCT
    out = []
    a = first
    while a < first + n:
        pe = min(first + n, a + pool)
        if nqt < HEAD_TAIL_NQT and not forced and pe - a >= HEAD_TAIL_POOL:
            pre = PRE if (nqt < PRE_NQT and pe - a >= PRE_POOL) else 0
            mid = pe - a - HEAD - TAIL - pre
            nm = max(1, (mid + sub // 2) // sub)
            each = _r64((mid + nm - 1) // nm)
            out.append((a, HEAD, True))
            x = a + HEAD
            while x < pe - TAIL - pre:
                out.append((x, min(each, pe - TAIL - pre - x), False))
                x += each
            if pre:
                out.append((pe - TAIL - pre, pre, False))
            out.append((pe - TAIL, TAIL, False))
        else:
            ln = pe - a
            ns = max(1, (ln + sub // 2) // sub)
            each = _r64((ln + ns - 1) // ns)
            if 0 < first_pct < 100 and ns >= FIRST_MIN_SLICES and not forced:
                first_n = max(64, each * first_pct // 100 // 64 * 64)
                each2 = _r64((ln - first_n + ns - 2) // (ns - 1))
                out.append((a, first_n, True))
                x = a + first_n
                while x < pe:
                    out.append((x, min(each2, pe - x), False))
                    x += each2
            else:
                x = a
                while x < pe:
                    out.append((x, min(each, pe - x), x == a))
                    x += each
        a += pool
    return out


# ---- the cases: name -> queries, references, pool (None: all), a constant-and-complete column or none, the lengths the planner must give, its rules
Case = collections.namedtuple("Case", "nq n pool cons lengths rules")
CASES = collections.OrderedDict([
    ("a", Case(5, 163877, None, True, (38208, 62848, 62821), "query-tile scaling, quarter rule, 70 % first slice")),
    ("b", Case(5, 524325, None, True, (HEAD, 131136, 131136, 130981, TAIL), "head / middle / tail; the last middle ends off a tile boundary")),
    ("c", Case(5, 786469, None, True, (HEAD, 174784, 174784, 174757, PRE, TAIL), "head / middle / pre / tail")),
    ("d", Case(49, 524325, None, True, (HEAD, 196672, 196581, TAIL), "head / middle / tail over the column-compressed scan, no pre")),
    ("e", Case(5, 600037, 300000, True, (52480, 82560, 82560, 82400) * 2 + (37,), "two pools of four slices with a 70 % first one, a pool of 37: plain near-equal slices")),
    ("f", Case(5, 600037, 300000, False, (HEAD, 156352, 156352, 156261, TAIL), "the pool is ignored without a constant-and-complete column")),
    ("g", Case(1000, 62757, None, True, (14592, 24128, 24037), "63 query tiles: no scaling, 70 % first slice")),
])

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.zeros(256, dtype=np.uint8)
_CODE[_ACGT] = np.arange(4)
P_COLS = np.arange(12) * 10 + 3          # the columns the queries differ at
M_COLS = np.array([120, 121])            # N in the second query: constant, not complete
E_COLS = np.setdiff1d(np.arange(NCHAR), np.concatenate([P_COLS, M_COLS]))          # the columns a reference's deficits go to
HIGH_START, HIGH_END = 10, 7             # substitutions of a reference on its step, at the two ends of the stream
LOW_START = 3                            # substitutions of the first references of a step, at the start of the stream (0 at its end): at least four
                                         # below HIGH, so that a snapshot taken under them, whatever a query adds at its own columns, is below HIGH
LOWS_PER_STEP = 2
NOISE_BELOW = 3                          # noise is worse than its step by more than a query's own letters can make good (three columns at the most)
PAIR_DEFICITS = 10                       # pair k has k sites N and nothing else: better than every step of the staircase, which keeps this many and more
STEP = 7000                              # references of a step of the staircase (below WINDOW: the first of a step's own references is always admitted)
MAX_LEVELS = 105


def case_pool(key):
    c = CASES[key]
    return c.pool or c.n


def case_plan(key, acgt, n_idx_c):
    c = CASES[key]
    return plan(0, c.n, case_pool(key), c.nq, n_idx_c, acgt)


@functools.lru_cache(maxsize=None)
def make_queries(nq, cons):
    """nq distinct query rows (uint8 [nq, NCHAR]) and the root they are made from: the root with one to three other letters at P_COLS; with cons
    the second query misses M_COLS, without it every column misses in one query, so that none is constant and complete"""
    rng = np.random.default_rng(4100 + nq + (0 if cons else 1))
    root = _ACGT[rng.integers(0, 4, NCHAR)]
    seen, out = set(), []
    j = 0
    while len(out) < nq:
        a = root.copy()
        cols = rng.choice(P_COLS, size=1 + j % 3, replace=False)
        a[cols] = _ACGT[(_CODE[a[cols]] + rng.integers(1, 4, len(cols))) % 4]
        j += 1
        if a.tobytes() in seen:
            continue
        seen.add(a.tobytes())
        out.append(a)
    Q = np.array(out)
    if cons:
        Q[1 % nq, M_COLS] = ord("N")
    else:
        for j in range(nq):
            Q[j, j::nq] = ord("N")
    return Q, root


def query_rows(key):
    return make_queries(CASES[key].nq, CASES[key].cons)


@functools.lru_cache(maxsize=None)
def query(key, acgt):
    Q, _ = query_rows(key)
    return O.Query([r.tobytes() for r in Q], ["q%d" % i for i in range(len(Q))], acgt=acgt, ambig_q=1.0)


def boundaries(key):
    """where the slices of a case's plan meet (the plan does not depend on the mode for these query sets)"""
    c = CASES[key]
    pl = plan(0, c.n, case_pool(key), c.nq, 1 if c.cons else 0, False)
    assert tuple(s[1] for s in pl) == c.lengths, (key, pl)
    return [s[0] for s in pl[1:]]


@functools.lru_cache(maxsize=None)
def refs(key):
    """the references of a case: uint8 [n, NCHAR]"""
    c = CASES[key]
    Q, root = query_rows(key)
    n = c.n
    rng = np.random.default_rng(7700 + n)
    levels = max(8, min(MAX_LEVELS, -(-n // STEP)))
    step = -(-n // levels)
    i = np.arange(n)
    level = i // step
    on_step = rng.random(n) < 0.12
    on_step[np.minimum(level * step + 1, n - 1)] = True                  # (a step's low references come early)
    nth = np.cumsum(on_step) - np.concatenate([[0], np.cumsum(on_step)[step - 1::step]])[level]          # 1, 2, ... over a step's own references
    high = HIGH_END + np.rint((HIGH_START - HIGH_END) * (1 - i / n)).astype(np.int64)
    low = np.rint(LOW_START * (1 - level / (levels - 1))).astype(np.int64)
    deficit = PAIR_DEFICITS + (levels - 1 - level) + np.where(on_step, 0, NOISE_BELOW + rng.geometric(0.25, n))
    deficit = np.minimum(deficit, len(E_COLS))
    mis = np.where(on_step, np.where(nth <= LOWS_PER_STEP, low, high), high + rng.integers(0, 4, n))
    mis = np.minimum(mis, deficit)
    start = rng.integers(0, len(E_COLS), n)
    src = np.where(on_step, -1, rng.integers(0, c.nq, n))                # whose letters a reference carries at the queries' own columns (-1: the root's)
    shift = rng.integers(1, 4, (n, 1), dtype=np.uint8)
    b = boundaries(key)
    for k, x in enumerate(b):                                            # the pairs
        for r in (x - 1, x):
            deficit[r], mis[r], start[r], src[r] = k, 0, 0, -1
    perm = np.random.default_rng(99).permutation(len(E_COLS))
    pos = np.full(NCHAR, 1000, dtype=np.int16)                           # rank of a column in the order deficits are dealt in; no rank off E_COLS
    pos[E_COLS[perm]] = np.arange(len(E_COLS))
    root_code = _CODE[root]
    out = np.empty((n, NCHAR), dtype=np.uint8)
    for a in range(0, n, 65536):
        z = slice(a, min(n, a + 65536))
        rank = pos[None, :] - start[z, None].astype(np.int16)
        rank += (rank < 0) * np.int16(len(E_COLS))
        m, d = mis[z, None].astype(np.int16), deficit[z, None].astype(np.int16)
        blk = _ACGT[(root_code[None, :] + shift[z] * (rank < m)) & 3]
        blk[(rank >= m) & (rank < d)] = ord("N")
        from_q = np.nonzero(src[z] >= 0)[0]
        own = Q[src[z][from_q]][:, P_COLS]
        blk[np.ix_(from_q, P_COLS)] = np.where(own == ord("N"), root[P_COLS], own)
        out[z] = blk
    return out


_NAMES = []


def names(n):
    while len(_NAMES) < n:
        _NAMES.extend("r%d" % i for i in range(len(_NAMES), max(n, 2 * len(_NAMES))))
    return _NAMES[:n]


def run_oracle(key, acgt, pool=None, n=None):
    """the oracle over the first n references of a case (None: all) in batches of pool (None: the case's)"""
    c = CASES[key]
    n = c.n if n is None else n
    rows = [r.tobytes() for r in refs(key)[:n]]
    return O.search(query(key, acgt), rows, names(n), pool=pool or case_pool(key), nbest=NBEST, ambig_r=1.0, chunk=65536)


@functools.lru_cache(maxsize=None)
def gold(key, acgt):
    """the oracle's answer, computed once per (case, mode) and not changed afterwards; ambig_r = 1: no reference is filtered"""
    return run_oracle(key, acgt)


def longest_gap(saved, n):
    """the longest run of stream positions without an admission"""
    edges = np.concatenate([[-1], np.asarray(saved, dtype=np.int64), [n]])
    return int(np.diff(edges).max()) - 1


def want_rows(g):
    return [[(tuple(s), o) for o, _, s in rows] for rows in g.rows]


# ---- the schedule shape (sections "the schedule knobs change nothing" and "rebuild chunks that share tiles")
KNOB_NQ, KNOB_NREF, KNOB_NCHAR, KNOB_POOL, KNOB_NBEST = 70, 3000, 2300, 128, 5        # 24 pools of two tiles: every counter buffer is used six times
KNOB_CUT = 1301                                        # the database is loaded in two appends, the second starts inside a tile
CHUNK_NREF, CHUNK_POOL, CHUNK_CUT = 1000, 100, 333     # max_pool 100: the rebuild runs in ten chunks, nine of them begin inside a tile


@functools.lru_cache(maxsize=None)
def knob_inputs(acgt):
    """(prepared query, reference rows) of the schedule shape: a synthetic alignment shaped like SARS-CoV-2 data"""
    import fixtures as F
    refs_, root, cols = F.synth_alignment(KNOB_NREF, KNOB_NCHAR, seed=5100)
    qs, _, _ = F.synth_alignment(KNOB_NQ, KNOB_NCHAR, seed=5101, root=root, poly_cols=cols, p_snp=0.004, p_amb=0.002)
    return O.Query(qs, ["q%d" % i for i in range(len(qs))], acgt=acgt), refs_


@functools.lru_cache(maxsize=None)
def knob_gold(acgt, n=KNOB_NREF, pool=KNOB_POOL):
    q, refs_ = knob_inputs(acgt)
    return O.search(q, refs_[:n], names(n), pool=pool, nbest=KNOB_NBEST, ambig_r=1.0)
