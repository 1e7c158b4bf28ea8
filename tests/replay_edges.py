"""Inputs that take the ordered gate / heap replay (kernels_replay.inc: replay_kernel, replay2_kernel, replay2_lean_kernel, replay3_kernel, chosen
by launch_replay in host_launch.inc) to its edges -- walks of the tile bounds over one, PD, 9, BR and 2 BR + 1 rounds, a skipped tile that
becomes needed after the tolerance rose, heaps whose entries tie on all six keys so that only the layout of src/min_heap.c decides who is
evicted, candidates that tie the worst kept entry on keys 0..j-1 and differ by one at key j, tolerances on both sides of every entry of
TB8_THR, ambiguity-word lists of exactly AMB_CAP and AMB_CAP + 1 words, ordinals with a high word, the last alignment length of the 16-bit
scan, consensus pre-scores cut at the batch snapshot in every word, bit and lane position of the cut walk -- and a small model (MinHeap,
walk2, walk3, cut_walk) that says which edge an input reaches.  The model never judges a result: the oracle does.
Deterministic and seeded; no GPU code here.  tests/test_replay_edges_cpu.py shows that every input reaches the edge it is built for,
tests/test_replay_edges_gpu.py runs the inputs on the device.

The edge table: which line each group is aimed at (kernels_replay.inc unless another file is named).
  R  rounds of tile bounds, the ring   replay2_kernel / replay2_lean_kernel (replay_bounds_start, replay_bounds_next): `nbq[i] = tmrow[i * 64 + lane];`  `for (int i = 0; i + 1 < PD; i++) nbq[i] = nbq[i + 1];`
                                       `if (use_tmin && tb + PD * 64 + lane < n_slice_tiles) nbq[PD - 1] = tmrow[tb + PD * 64 + lane];`
                                       replay3_kernel: `lds_dma_dwordx4(src, bring_lds + (uint32_t)(r & (BR - 1)) * 1024u);`  `for (int r = 0; r < 9; r++) fetch_bounds(r);`
                                       `if ((rnd & 3) == 3) {`  `for (int r = rnd + 6; r < rnd + 10; r++) fetch_bounds(r);`  `const uint4 tbv = bring[(rnd & (BR - 1)) * 64 + lane];`
                                       `have[0] = needed(bring[((rnd + 1) & (BR - 1)) * 64 + lane]) & SUB0;`  `const uint4 *src = t < n_slice_tiles ? tmrow + t : &g_replay_zero16;`
                                       host_resident.inc: `if (c->subslice_forced) sub = std::min(pool, c->subslice);` (one slice per run)
  G  a skipped tile becomes needed     replay2_kernel: `if (T > T_used && last >= 0 && (P & ~inflight & ((1ull << last) - 1ull)) != 0ull) regroup = true;`  `else P |= inflight;`
                                       replay2_lean_kernel: `if (T > T_used && G && (P & ~G & ((1ull << (63 - __clzll((long long)G))) - 1ull)) != 0ull) break;`  `P |= G;`
                                       replay3_kernel: `if (!((have[b] >> tsel) & 1ull)) {`  `if (hb + 1 < NSUB) { have[b ^ 1] = needed(tbv) & (SUB0 << (HALF * (hb + 1)));`
                                       `if (admitted_here || T != T_used) P = needed(tbv) & half_mask & ~((2ull << tsel) - 1ull);`
  H  heap layout                       `static __device__ __forceinline__ int wave_minchild_init(` : `if (better) mcv = c + 1;`  wave_replace_root_mc: `if (D == d && ahead) D = d + 1;`
                                       `if (lane == nd) mc = left_ahead ? cc + 1 : cc;`  replay_heap_state: `const bool use_mc = k <= 127;`  wave_replace_root: `p = b2 ? c + 1 : c;`
                                       heap_sift_down (replay_kernel): `if (c + i <= n && lex_better(h + pick * HEAP_ENTRY, h + (c + i) * HEAP_ENTRY)) pick = c + i;`  wave_sift_up
                                       replay_admit (the other three kernels): `if (!(was_full && use_mc)) replay_worst_keys<LEAN>(h, W);`  `if (!was_full && use_mc) mc = wave_minchild_init(h, n, lane);`
  K  the key ladder                    `static __device__ __forceinline__ bool lex_better(`  replay2_kernel may_enter: `return K3[u] >= W[3];`  `return K0[u] >= W[0];`
                                       replay_kernel, replay_exact_default: `const bool accept = (mi < T) && (!full || lex_better(Si, W));`  `mask = __ballot(lane > i && may_enter());`  replay3_kernel: `return lex_better(S, W);`
  T  the tolerance and the bounds      replay3_kernel needed: `for (int i = TB8_N - 2; i >= 0; i--) if (TB8_THR[i] >= T - 1) j = i;`  `return __ballot(e != 0u && (!full || (int)e > W[0]));`
                                       kernels_scan2.inc: `__device__ constexpr int TB8_THR[TB8_N - 1] = {0, 1, 2, 3, 5, 8, 14};`  tile_bounds8: `(in_batch && (j == TB8_N - 1 || mm <= TB8_THR[j]))`
                                       replay2_kernel needed: `return __ballot((tm < T || (CONS && snap < T)) && (!full || tk >= W[0]));`
  S  slow pairs                        wave_iupac_request: `if (nq <= AMB_CAP) {`  `} else if (lane < nq + AMB_CAP) {`  wave_iupac_finish: `dense = (nr > AMB_CAP || nq > AMB_CAP);`
                                       `const bool mine = lane < nq || (lane < nq + nr && !((qlisted[e.w >> 5] >> (e.w & 31)) & 1u));`  replay3_kernel: `const bool slow = cut || xraw == EXT_UNKNOWN;`
                                       `if (slow) return K0 >= W[0];`  `const bool cut = CONS && mc_true >= snap;`  kernels_scan2.inc: `ext[(size_t)q * ppad + r] = (r_known && aqn[i] <= AMB_CAP) ?`
  F  range ends                        replay_kernel: `e[6] = (int)(unsigned)(ord & 0xffffffffll); e[7] = (int)(ord >> 32);`  replay_admit: `if ((lane & 7) == 7) v = (int)(ord >> 32);`  `const long long ord = ord_base + (rl - r_begin);`
                                       `const bool valid = (base_u + lane >= r_begin) && (base_u + lane < r_end);`  host_open.inc: `if (c->nchar > 49000) c->fullscan = true;`
                                       `return !c ? -2 : c->fullscan ? -1 : c->scan_variant;`  host_launch.inc: `if (c->fullscan) {` of launch_replay, `bool lean = lean_replay_context(c) && L.prefetch == 2 && lq_words == 0;`
                                       host_open.inc: `c->use_ext = !c->fullscan && !c->acgt && tn.replay_extras != 1 && (c->scan_variant == 0 ||`  `c->replay_half = (want_half == 32 || want_half == 16 || want_half == 8) ? want_half : c->nq <= 8 ? 32 : c->nq <= 24 ? 16 : 8;`
  C  the cut of the pre-score         kernels_consensus.inc, wave_truncated_consensus: `const int NW = W4 * 4, B = (NW + 63) / 64;`  `const int w_lo = min(lane * B, NW), w_hi = min(w_lo + B, NW);`
                                       `for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }`  `const unsigned long long reach = __ballot(snap > 0 && incl >= snap);`
                                       `int mcur = excl;`  `if (mcur + pw >= snap) {`  `const uint32_t pmask = prefix_through_nth_bit(M, snap - mcur);`  `for (int k = 1; k < nth; k++) m &= m - 1;`
                                       `r[3] = dbw[base + (size_t)(P - 1) * 256];`  consensus_kernel: `if (!done && mcur + pm >= snap) {`  `const uint32_t pmask = prefix_through_nth_bit(M, snap - mcur);`
                                       replay_kernel: `const int4 rc = (mc_true >= snap) ? tr[r] : a;`  replay2_kernel: `cut[u] = CONS && mc_true >= snap;`  `m[u] = K3[u] - K0[u] - (cut[u] ? mc_true - snap : 0);`
                                       `if (cut[u]) return K0[u] >= W[0];`  replay3_kernel: `const int m = V - K0 - (cut ? mc_true - snap : 0);`  host_open.inc: `c->W = (c->nchar + 31) / 32; c->W4 = (c->W + 3) / 4;`"""
import collections
import functools

import numpy as np

import oracle_lib as O

# ---- copies of the code's constants; each moves with the line it mirrors
D = 8                        # `constexpr int D = 8;`  tiles of replay2_kernel / replay2_lean_kernel in flight
PD = 4                       # `constexpr int PD = 4;`  rounds of bounds those two request ahead
BR = 16                      # `constexpr int BR = 16;`  rounds of bounds in replay3_kernel's LDS ring
INITIAL_ROUNDS = 9           # `for (int r = 0; r < 9; r++) fetch_bounds(r);`
TB8_THR = (0, 1, 2, 3, 5, 8, 14)   # `__device__ constexpr int TB8_THR[TB8_N - 1] = {0, 1, 2, 3, 5, 8, 14};` (kernels_scan2.inc)
AMB_CAP = 11                 # `constexpr int AMB_CAP = 11;` (uvaia_gpu.hip)
MC_LIMIT = 127               # `const bool use_mc = k <= 127;`
WIDE_ABOVE = 49000           # `if (c->nchar > 49000) c->fullscan = true;` (host_open.inc)
TILE = 64                    # references of a tile, tiles of a round of bounds
LEAN_NQ = 256                # `if (c->replay_lq < 0) c->replay_lq = (nq < 256) ? 1 : 0;` (host_qprep.inc) and `const int pf = (q1 - q0) <= 64 ? 1 : 2;` (host_resident.inc)

_ROT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    _ROT[_a] = _b


def rot(a, k=1):
    """every A, C, G, T moved k letters on (A -> C -> G -> T -> A); other bytes stay"""
    a = np.asarray(a, dtype=np.uint8)
    for _ in range(k):
        a = _ROT[a]
    return a


def make_root(nchar, seed):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), nchar)


def edit(base, subs=(), to_n=(), put=None):
    """a copy of `base` (uint8 array) with the columns `subs` moved one letter on, the columns `to_n` set to N, and put = {column: byte}"""
    a = np.array(base, dtype=np.uint8)
    subs = list(subs)
    if subs:
        a[subs] = _ROT[a[subs]]
    to_n = list(to_n)
    if to_n:
        a[to_n] = ord("N")
    for c, b in (put or {}).items():
        a[c] = b if isinstance(b, int) else ord(b)
    return a


def rows(a):
    """list of bytes rows of a 2-D uint8 array or of a list of 1-D arrays"""
    return [np.asarray(r, dtype=np.uint8).tobytes() for r in a]


def far_rows(root, n, n_mis, seed, cols=None):
    """n references that differ from root in n_mis columns each (drawn among `cols`), by one, two or three letters: a uint8 array [n, nchar]"""
    rng = np.random.default_rng(seed)
    cols = np.arange(len(root)) if cols is None else np.asarray(cols)
    out = np.tile(np.asarray(root, dtype=np.uint8), (n, 1))
    if n == 0:
        return out
    pick = cols[np.argsort(rng.random((n, len(cols))), axis=1)[:, :n_mis]]
    r = np.repeat(np.arange(n), n_mis)
    c = pick.reshape(-1)
    v = out[r, c]
    k = rng.integers(1, 4, size=v.shape)
    for step in (1, 2, 3):
        v = np.where(k >= step, _ROT[v], v)
    out[r, c] = v
    return out


def names(n, p="r"):
    return ["%s%d" % (p, i) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ kernel regimes
# how launch_replay comes to each kernel (host_open.inc, host_launch.inc, host_resident.inc): mode, tuning, push or resident search, number of queries
Regime = collections.namedtuple("Regime", "acgt tuning path nq kernel")
REGIMES = {
    "replay3": Regime(False, {}, "push", None, "replay3"),                                   # at most 32 queries: HALF 32 / 16 / 8 by their number
    "replay3-h32": Regime(False, {"replay_cus": 32008}, "push", None, "replay3"),
    "replay3-h16": Regime(False, {"replay_cus": 16008}, "push", None, "replay3"),
    "replay3-h8": Regime(False, {"replay_cus": 8008}, "push", None, "replay3"),
    "replay3-res-h32": Regime(False, {"replay_cus": 32008}, "resident", None, "replay3"),
    "replay3-res-h16": Regime(False, {"replay_cus": 16008}, "resident", None, "replay3"),
    "replay3-res-h8": Regime(False, {"replay_cus": 8008}, "resident", None, "replay3"),
    "replay2": Regime(False, {"replay_extras": 1}, "push", None, "replay2"),               # PF = 3 through push
    "replay2-res": Regime(False, {"replay_extras": 1}, "resident", None, "replay2"),       # PF = 1: at most 64 queries, resident
    "replay2-acgt": Regime(True, {}, "push", None, "replay2"),
    "replay2-acgt-res": Regime(True, {}, "resident", None, "replay2"),
    "lean": Regime(False, {}, "resident", LEAN_NQ, "lean"),                                  # 256 queries, no constant-and-complete column, nbest <= 127
    "replay2-q256": Regime(False, {}, "resident", LEAN_NQ, "replay2"),                       # the same query set with nbest > 127: replay2_kernel, PF = 2
    "wide": Regime(False, {"scan": "wide"}, "push", None, "replay"),
    "wide-res": Regime(False, {"scan": "wide"}, "resident", None, "replay"),
    "wide-acgt": Regime(True, {"scan": "wide"}, "push", None, "replay"),
    "auto": Regime(False, {}, "push", None, None),                                           # the library's choice: what group F's lengths switch
    "auto-acgt": Regime(True, {}, "push", None, None),
}


def fillers(root, n, cols=None):
    """n queries, each the root with two private substitutions; with n >= 64 every column of `cols` differs in some query (no constant column)"""
    cols = np.arange(len(root)) if cols is None else np.asarray(cols)
    out = []
    for i in range(n):
        a = np.array(root, dtype=np.uint8)
        c1, c2 = cols[i % len(cols)], cols[(i * 7 + 3) % len(cols)]
        k = 1 + (i // len(cols)) % 3
        a[c1] = rot(a[c1:c1 + 1], k)[0]
        if c2 != c1:
            a[c2] = rot(a[c2:c2 + 1], k)[0]
        out.append(a)
    return out


Case = collections.namedtuple("Case", "name group queries refs nbest pool regimes meta")
# name: the edge (`tiles1025`); queries[0] is the probe; regimes: names of REGIMES the device test runs it under; a regime with nq = 256 gets
# the probe followed by fillers (queries_for)


def queries_for(case, regime):
    """the query rows of a case under a regime: its own, or (a regime of 256 queries) its probes plus fillers that leave no constant column"""
    r = REGIMES[regime]
    if r.nq is None:
        return rows(case.queries)
    base = case.meta.get("filler_root", case.queries[0])
    return rows(list(case.queries) + fillers(base, r.nq - len(case.queries), case.meta.get("filler_cols")))


@functools.lru_cache(maxsize=None)
def _query(key, regime):
    case = CASES[key]
    seqs = queries_for(case, regime)
    return O.Query(seqs, names(len(seqs), "q"), trim=case.meta.get("trim", 0), acgt=REGIMES[regime].acgt, ambig_q=1.0)


def query(key, regime):
    """the oracle's prepared query of a case under a regime (cached; regimes of the same mode and size share it)"""
    r = REGIMES[regime]
    canon = next(n for n, x in REGIMES.items() if x.acgt == r.acgt and x.nq == r.nq)
    return _query(key, canon)


@functools.lru_cache(maxsize=None)
def _gold(key, canon):
    case = CASES[key]
    refs = list(case.refs)
    if "range" in case.meta:                                  # a pool inside the database: the oracle sees those references alone
        refs = refs[case.meta["range"][0]:sum(case.meta["range"])]
    return O.search(_query(key, canon), refs, names(len(refs)), pool=case.pool, nbest=case.nbest, ambig_r=1.0)


def gold(key, regime):
    """the oracle's answer, computed once per (case, mode, number of queries) and not changed afterwards; ambig_r = 1: no reference is filtered"""
    r = REGIMES[regime]
    canon = next(n for n, x in REGIMES.items() if x.acgt == r.acgt and x.nq == r.nq)
    return _gold(key, canon)


def probe_index(key, regime):
    """the oracle orders a query set its own way: where the probe (queries[0]) sits in the prepared set"""
    return query(key, regime).seqs.index(rows(CASES[key].queries[:1])[0])


def want_rows(g, ntax, ordinal0=0):
    return [[(tuple(s), o + ordinal0) for o, _, s in g.rows[iq]] for iq in range(ntax)]


# ------------------------------------------------------------------------------------------------------------------ the model
def lex_better(a, b):
    """compare_q_item_score(a, b) < 0 (src/min_heap.c:41-47): a ranks strictly ahead of b -- larger keys first"""
    for x, y in zip(a, b):
        if x != y:
            return x > y
    return False


def mismatches(s, acgt=False):
    return s[1] - s[0] if acgt else s[3] - s[0]              # src/nearest.c:475 / :508


class MinHeap:
    """heap_insert, heap_bubble_up, heap_bubble_down of src/min_heap.c:93-147 on (scores, ordinal) entries; the root (slot 1) is the worst kept
    entry.  prefer_right = True is the WRONG rule for equal children (the right one), kept to show that the inputs can tell the two apart."""

    def __init__(self, nbest, prefer_right=False):
        self.k = max(2, nbest)                             # src/min_heap.c:58
        self.e = [None]
        self.prefer_right = prefer_right
        self.depths = []                                   # levels below the root at which each root replacement came to rest
        self.tied_evictions = 0                            # replacements whose evicted root tied another kept entry on all six keys

    @property
    def n(self):
        return len(self.e) - 1

    @property
    def full(self):
        return self.n == self.k

    def tolerance(self, nchar, acgt=False):
        return mismatches(self.e[1][0], acgt) + 1 if self.full else nchar

    def _down(self, p):
        depth = 0
        while True:
            c, pick = 2 * p, p
            order = (c + 1, c) if self.prefer_right else (c, c + 1)
            for x in order:
                if x <= self.n and lex_better(self.e[pick][0], self.e[x][0]):
                    pick = x
            if pick == p:
                return depth
            self.e[p], self.e[pick] = self.e[pick], self.e[p]
            p = pick
            depth += 1

    def insert(self, scores, ordinal):
        scores = tuple(int(x) for x in scores)
        if self.full:
            if not lex_better(scores, self.e[1][0]):
                return False
            if any(x[0] == self.e[1][0] for x in self.e[2:]):
                self.tied_evictions += 1
            self.e[1] = (scores, ordinal)
            self.depths.append(self._down(1))
            return True
        self.e.append((scores, ordinal))
        i = self.n
        while i > 1 and lex_better(self.e[i // 2][0], self.e[i][0]):
            self.e[i // 2], self.e[i] = self.e[i], self.e[i // 2]
            i //= 2
        return True

    def final(self):
        """heap_finalise_heap_qsort (src/min_heap.c:149-158): slot n to the front, then a stable sort, best first"""
        k = self.n
        order = ([k] + list(range(1, k))) if k else []
        out = [self.e[s] for s in order]
        out.sort(key=lambda r: tuple(-v for v in r[0]))
        return out


def replay_model(scores, nbest, nchar, prefer_right=False, acgt=False):
    """The search of ONE query over untruncated score vectors (valid where no pre-score is cut: a single pool, or no constant-and-complete
    column): src/nearest.c:488-508.  Returns the heap and, per reference, (entered, tolerance after it, worst kept key 0 after it).
    What a cut pair's pre-score holds, and where its walk stops, is cut_walk's business (group C)."""
    h = MinHeap(nbest, prefer_right)
    trace = []
    for o, s in enumerate(scores):
        ent = mismatches(s, acgt) < h.tolerance(nchar, acgt) and h.insert(s, o)
        trace.append((bool(ent), h.tolerance(nchar, acgt), h.e[1][0][0] if h.full else None))
    return h, trace


def tile_bounds(scores, acgt=False):
    """per tile: (smallest mismatch count, largest key 0) as scan2_finish leaves them in tmin, and the eight entries of tile_bounds8"""
    s = np.asarray(scores)
    mm = (s[:, 1] - s[:, 0]) if acgt else (s[:, 3] - s[:, 0])
    k0 = s[:, 0]
    out = []
    for a in range(0, len(s), TILE):
        m, k = mm[a:a + TILE], k0[a:a + TILE]
        e = [int(k[m <= thr].max()) + 1 if (m <= thr).any() else 0 for thr in TB8_THR] + [int(k.max()) + 1]
        out.append((int(m.min()), int(k.max()), e))
    return out


def tb8_index(T):
    """`for (int i = TB8_N - 2; i >= 0; i--) if (TB8_THR[i] >= T - 1) j = i;`: the smallest threshold >= T - 1, else the last entry"""
    j = len(TB8_THR)
    for i in range(len(TB8_THR) - 1, -1, -1):
        if TB8_THR[i] >= T - 1:
            j = i
    return j


class _State:
    """the probe's heap state walked tile by tile: admits in lane order by the exact test"""

    def __init__(self, scores, nbest, nchar):
        self.s, self.h, self.nchar = scores, MinHeap(nbest), nchar
        self.entered = []

    @property
    def T(self):
        return self.h.tolerance(self.nchar)

    def w0(self):
        return self.h.e[1][0][0] if self.h.full else None

    def open(self, tile):
        for o in range(tile * TILE, min(len(self.s), (tile + 1) * TILE)):
            if mismatches(self.s[o]) < self.T and self.h.insert(self.s[o], o):
                self.entered.append(o)


def walk2(scores, nbest, nchar):
    """The walk of replay2_kernel / replay2_lean_kernel over one slice, default mode, no pre-score: which tiles are requested in groups of D,
    where the group is formed again after the tolerance rose (`regroup`), where the tolerance fell under tiles in flight (`fell`: tiles in
    flight that the new state no longer needs).  Returns (entered ordinals, regroups [(tile that raised, tile that became needed, tiles in flight behind it)],
    fells [(tile, tiles in flight no longer needed)], tiles opened)."""
    st = _State(scores, nbest, nchar)
    tb = tile_bounds(scores)
    regroups, fells, opened = [], [], []
    for r0 in range(0, len(tb), TILE):
        rt = tb[r0:r0 + TILE]

        def needed():
            return {i for i, (tm, tk, _e) in enumerate(rt) if tm < st.T and (not st.h.full or tk >= st.w0())}
        P = needed()
        while P:
            group = sorted(P)[:D]
            regroup = False
            for gi, t in enumerate(group):
                if regroup:
                    break
                T_used = st.T
                st.open(r0 + t)
                opened.append(r0 + t)
                P.discard(t)
                if st.T != T_used:
                    P = {x for x in needed() if x > t}
                    inflight = set(group[gi + 1:])
                    last = max(inflight) if inflight else -1
                    early = {x for x in P - inflight if x < last}
                    if st.T > T_used and last >= 0 and early:
                        regroup = True
                        regroups.append((r0 + t, r0 + min(early), len(inflight)))
                    else:
                        if st.T < T_used and inflight - P:
                            fells.append((r0 + t, sorted(r0 + x for x in inflight - P)))
                        P |= inflight
    return st.entered, regroups, fells, opened


def walk3(scores, nbest, nchar, half):
    """The walk of replay3_kernel<false, half> over one slice without slow pairs: the counters of a half round are requested one half ahead for
    the tiles the state of that moment would open; a tile that is needed when its turn comes and was not requested is fetched late.
    Returns (entered ordinals, tiles fetched late, tiles opened)."""
    st = _State(scores, nbest, nchar)
    tb = tile_bounds(scores)
    n_rounds = (len(tb) + TILE - 1) // TILE
    nsub = TILE // half

    def needed(rnd, lo, hi):
        j = tb8_index(st.T)
        out = set()
        for t in range(rnd * TILE + lo, min(len(tb), rnd * TILE + hi)):
            e = tb[t][2][j]
            if e != 0 and (not st.h.full or e > st.w0()):
                out.add(t)
        return out
    have = [needed(0, 0, half), set()]
    late, opened = [], []
    for rnd in range(n_rounds):
        for hb in range(nsub):
            b = hb & 1
            if hb + 1 < nsub:
                have[b ^ 1] = needed(rnd, half * (hb + 1), half * (hb + 2))
            elif rnd + 1 < n_rounds:
                have[0] = needed(rnd + 1, 0, half)
            P = needed(rnd, half * hb, half * (hb + 1))
            while P:
                t = min(P)
                P.discard(t)
                if t not in have[b]:
                    late.append(t)
                    have[b].add(t)
                opened.append(t)
                T_used, n_in = st.T, len(st.entered)
                st.open(t)
                if len(st.entered) != n_in or st.T != T_used:
                    P = {x for x in needed(rnd, half * hb, half * (hb + 1)) if x > t}
    return st.entered, late, opened


def _byte_table(chars, value=True, dtype=bool):
    t = np.zeros(256, dtype=dtype)
    for c in chars:
        t[c] = value
    return t


_IS_ACGT = _byte_table(b"ACGTacgt")                               # src/utils.c:262
_IS_INVALID = _byte_table(b"NnXx-?Oo.")                           # src/utils.c:263
_IUPAC = np.zeros(256, dtype=np.uint8)
for _c, _m in zip(b"ACGTMRWSYKVHDB", (1, 2, 4, 8, 3, 5, 9, 6, 10, 12, 7, 11, 13, 14)):
    _IUPAC[_c] = _IUPAC[_c + 32] = _m

CUT_WRONG = ("early", "late", "word", "carry", "noidx")
CutWalk = collections.namedtuple("CutWalk", "cut counters col word bit lane pos mis_before mis_after match_after")


def lane_split(nchar):
    """(W4, NW, B, lanes that hold words) of wave_truncated_consensus: `c->W = (c->nchar + 31) / 32; c->W4 = (c->W + 3) / 4;`,
    `const int NW = W4 * 4, B = (NW + 63) / 64;`, `const int w_lo = min(lane * B, NW), w_hi = min(w_lo + B, NW);`"""
    W4 = ((nchar + 31) // 32 + 3) // 4
    NW = 4 * W4
    B = (NW + 63) // 64
    return W4, NW, B, -(-NW // B)


def _as_u8(x):
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=np.uint8)


def cut_walk(consensus, idx_c, ref, snap, acgt, W4=None, wrong=None, every=None):
    """The consensus pre-score of one reference as src/nearest.c:428-433 leaves it with maxdist = snap: the sites of idx_c are walked in order
    and the walk stops right after the site at which the mismatch counter reaches snap.  Returns a CutWalk: cut (the counter reaches snap),
    counters (default: ACGT matches, text matches, partial matches, valid pairs; --acgt: mismatches, pairs of two ACGT, 0, 0), and where the
    cut falls: the column, its 32-site word and bit and -- given W4 -- the lane `word // B` of wave_truncated_consensus and the word's place
    in that lane's range ("first", "inner", "last", or "only" where the range is one word); the set bits of the word's mismatch plane before
    and after the cut bit, and the matching idx_c sites after it in the same word.  The model never judges a device result: the CPU test
    holds its counters against oracle_lib.score4 / score_acgt.
    wrong = one of CUT_WRONG gives the counters of a WRONG walk, kept to show that the inputs tell it from the right one: "early" / "late"
    stop one mismatch before / after, "word" counts the whole word of the cut, "carry" loses the mismatches of the lanes in front when it
    walks the lane of the cut (needs W4), "noidx" walks every column (against `every`, a query, where the consensus has no letter)."""
    cons, ref = _as_u8(consensus), _as_u8(ref)
    idx = np.asarray(idx_c, dtype=np.int64)
    if wrong == "noidx":
        cons = np.where(_IS_ACGT[cons], cons, _as_u8(every))
        idx = np.arange(len(ref), dtype=np.int64)
    a, b = ref[idx], cons[idx]
    zero = np.zeros(len(idx), dtype=bool)
    if acgt:
        both = _IS_ACGT[a] & _IS_ACGT[b]
        mis = both & (a != b)
        planes, match = (mis, both, zero, zero), both & (a == b)
    else:
        valid = ~_IS_INVALID[a] & ~_IS_INVALID[b]
        text = valid & (a == b)
        match = text & _IS_ACGT[a]
        planes, mis = (match, text, valid & ((_IUPAC[a] & _IUPAC[b]) != 0), valid), valid & ~match
    cum = np.cumsum(mis)
    n = len(idx)

    def stop_at(count, lo=0, hi=n):
        """sites walked when the walk over [lo, hi) stops right after its count-th mismatch (counted from lo)"""
        if count <= 0:
            return lo
        local = np.cumsum(mis[lo:hi])
        return lo + int(np.argmax(local >= count)) + 1 if len(local) and local[-1] >= count else hi
    cut = bool(n and cum[-1] >= snap)
    stop = stop_at(snap)
    where = (None,) * 8
    if cut:
        col = int(idx[stop - 1])
        w, bit = col // 32, col % 32
        in_w = (idx // 32) == w
        before, after = in_w & (idx < col), in_w & (idx > col)
        lane = pos = None
        if W4 is not None:
            NW = 4 * W4
            B = (NW + 63) // 64
            lane = w // B
            w_lo, w_hi = min(lane * B, NW), min(lane * B + B, NW)
            pos = "only" if w_hi - w_lo == 1 else "first" if w == w_lo else "last" if w == w_hi - 1 else "inner"
        where = (col, w, bit, lane, pos, int((mis & before).sum()), int((mis & after).sum()), int((match & after).sum()))
    if wrong == "early":
        stop = stop_at(snap - 1)
    elif wrong == "late":
        stop = stop_at(snap + 1)
    elif wrong == "word" and cut:
        stop = int(np.searchsorted(idx, 32 * (where[1] + 1)))
    elif wrong == "carry" and cut:
        B = (4 * W4 + 63) // 64
        lo, hi = (int(np.searchsorted(idx, 32 * B * (where[3] + d))) for d in (0, 1))
        stop = stop_at(snap, lo, hi)
    return CutWalk(cut, tuple(int(p[:stop].sum()) for p in planes), *where)


CASES = collections.OrderedDict()


def _add(case):
    key = "%s-%s" % (case.group, case.name)
    assert key not in CASES, key
    CASES[key] = case
    return key


def keys(group):
    return [k for k, c in CASES.items() if c.group == group]


def runs(group=None):
    """(case key, regime) of every device run, and its id `R-replay3-h16-tiles1025`"""
    out = []
    for k, c in CASES.items():
        if group is None or c.group == group:
            out += [(k, r) for r in c.regimes]
    return out


def run_id(key, regime):
    c = CASES[key]
    return "%s-%s-%s" % (c.group, regime, c.name)


class _Lazy:
    """references are built when first asked for (the largest stream is 135 168 rows) and kept"""

    def __init__(self, fn):
        self.fn, self.v = fn, None

    def get(self):
        if self.v is None:
            self.v = self.fn()
        return self.v


class _LazyList:
    """a list of rows that is built on first use"""

    def __init__(self, fn):
        self._l = _Lazy(fn)

    def __len__(self):
        return len(self._l.get())

    def __getitem__(self, i):
        return self._l.get()[i]

    def __iter__(self):
        return iter(self._l.get())


# ---------------------------------------------------------------------------------------------------------------------------- R
# Three queries (the probe is the root, the two others differ from it in two private columns each), 64 columns, heaps of 4.  The stream is
# N_t tiles of references some 30 mismatches away from every query; the `plants` -- lanes 0 .. 3 of the first tile (they fill the heaps,
# so nothing far ever enters), lanes 0 and 63 of the first and the last tile of the listed rounds, the stream's last reference -- have two
# mismatches, 10 + j matching columns and N elsewhere: plant j + 1 beats plant j on key 0 and displaces it, for every query.
R_NCHAR, R_NBEST, R_LAST = 64, 4, 37
R_ROUNDS = (0, 3, 4, 8, 9, 12, 13, 15, 16, 17, 31, 32)
R_TILES_2 = (1, 64, 65, 256, 257, 321)                      # one round | PD rounds | the first refill of nbq[PD - 1]
R_TILES_3 = R_TILES_2 + (576, 577, 833, 1024, 1025, 1089, 2112)   # 9 rounds requested up front | the refills at rounds 3, 7, 11 | BR slots | the second wrap
R_MIS, R_BASE = (0, 1), 10                                  # the plants' two mismatch columns; matching columns of plant 0 (columns 2 ..)
R_FILLER_COLS = ((2, 3), (4, 5))                            # inside the columns every plant matches


def r_plants(n_tiles):
    n = (n_tiles - 1) * TILE + R_LAST
    at = {0, 1, 2, 3, n - 1}
    for rnd in R_ROUNDS:
        if rnd * TILE < n_tiles:
            for t in (rnd * TILE, min(rnd * TILE + TILE - 1, n_tiles - 1)):
                at |= {t * TILE + lane for lane in (0, TILE - 1) if t * TILE + lane < n}
    return n, sorted(at)


def r_plant_row(root, j):
    m = R_BASE + j
    assert 2 + m <= R_NCHAR
    return edit(root, subs=R_MIS, to_n=range(2 + m, R_NCHAR))


def _r_refs(n_tiles):
    root = make_root(R_NCHAR, 101)
    n, at = r_plants(n_tiles)
    a = far_rows(root, n, 30, 1000 + n_tiles)
    for j, o in enumerate(at):
        a[o] = r_plant_row(root, j)
    return rows(a)


def _r_cases():
    root = make_root(R_NCHAR, 101)
    qs = [root] + [edit(root, subs=c) for c in R_FILLER_COLS]
    for nt in R_TILES_3:
        n, at = r_plants(nt)
        regs = []
        if nt <= 1089:
            regs += ["replay3-h32"]
            regs += ["replay3-h16", "replay3-h8"] if nt in (65, 577, 1025) else []
        if nt in (1025, 2112):
            regs += ["replay3-res-h32", "replay3-res-h16", "replay3-res-h8"]     # one slice: subslice_refs = the stream's length
        if nt in R_TILES_2:
            regs += ["replay2", "replay2-acgt", "lean", "wide"] + (["replay2-res"] if nt in (257, 321) else [])
        _add(Case("tiles%d" % nt, "R", qs, _LazyList(functools.partial(_r_refs, nt)), R_NBEST, n, regs,
                  {"n_tiles": nt, "plants": at, "n_ref": n}))


# ---------------------------------------------------------------------------------------------------------------------------- G
# 128 columns; the probe has N in the last 32 columns and a second query has N in the first 96, so no column is constant and complete and the
# probe's scores are the pair counters themselves.  Heaps of 2.  Round 0 fills the probe's heap with LOW (2 mismatches, 58 N: key 0 = 36, the
# root, T = 3) and NINE (9 mismatches, key 0 = 87).  In round 1 (or 2) tile u holds the plant (1 mismatch): it evicts LOW, the root becomes
# NINE and T jumps to 10.  Tile x holds a reference of 5 mismatches (key 0 = 91 >= 87): not needed before the jump under either kind of
# bound, needed after it.  Decoy tiles hold a copy of LOW: needed before the jump (2 < 3, key 0 = 36 >= 36), admitting nothing (equal on all
# six keys).  Every other reference is 40 mismatches away.
G_NCHAR, G_COLS, G_NBEST = 128, 96, 2


def _g_rows(root):
    cols = list(range(G_COLS))
    return {
        "low": edit(root, subs=cols[:2], to_n=cols[2:60]),
        "nine": edit(root, subs=cols[:9]),
        "nine2": edit(root, subs=cols[:9], to_n=cols[9:10]),
        "plant": edit(root, subs=cols[:1]),
        "five": edit(root, subs=cols[10:15]),
        "zero": np.array(root, dtype=np.uint8),
        "one": edit(root, subs=cols[20:21]),
    }


def _g_stream(layout, n_tiles):
    """layout: {tile: {lane: row name}}; built on first use"""
    return _LazyList(functools.partial(_g_build, dict(layout), n_tiles))


def _g_build(layout, n_tiles):
    root = make_root(G_NCHAR, 202)
    kinds = _g_rows(root)
    a = far_rows(root, n_tiles * TILE - 20, 40, 2000 + n_tiles, cols=np.arange(G_COLS))
    for t, lanes in layout.items():
        for lane, kind in lanes.items():
            a[t * TILE + lane] = kinds[kind]
    return rows(a)


def _g_cases():
    root = make_root(G_NCHAR, 202)
    qs = [edit(root, to_n=range(G_COLS, G_NCHAR)), edit(root, to_n=range(G_COLS))]
    fill = {0: {0: "low", 1: "nine"}}
    # ---- replay2 / lean: u = tile 66, decoys every second tile behind it
    for nd in (1, 7, 8):
        decoys = [68 + 2 * i for i in range(nd)]
        inflight_last = ([66] + decoys)[:D][-1]
        for place, x in (("between", 67), ("after", inflight_last + 1)):
            lay = dict(fill)
            lay[66] = {5: "plant"}
            for t in decoys:
                lay[t] = {9: "low"}
            lay[x] = {63: "five"}
            want = {"regroup": place == "between", "u": 66, "x": x, "decoys": nd}
            _add(Case("rise-%s-decoys%d" % (place, nd), "G", qs, _g_stream(lay, 130), G_NBEST, 130 * TILE - 20,
                      ["replay2", "lean", "replay2-res", "replay3-h32", "replay3-h8"], dict(want, filler_root=root)))
    # ---- replay3: the plant in half hb, x later in the same half | tile 0 of the following half | in the next round
    for half in (32, 16, 8):
        reg = ["replay3-h%d" % half, "replay2", "lean"]
        u = TILE + half + 1                                    # round 1, second half, its tile 1
        _add(Case("late-same-half-h%d" % half, "G", qs, _g_stream({**fill, u: {5: "plant"}, u + 3: {0: "five"}}, 200), G_NBEST, 200 * TILE - 20,
                  reg, {"late": "same-half", "half": half, "u": u, "x": u + 3, "filler_root": root}))
        u = TILE + half - 2                                    # round 1, first half; x = tsel 0 of the second half
        _add(Case("late-next-half-h%d" % half, "G", qs, _g_stream({**fill, u: {63: "plant"}, TILE + half: {0: "five"}}, 200), G_NBEST, 200 * TILE - 20,
                  reg, {"late": "next-half", "half": half, "u": u, "x": TILE + half, "filler_root": root}))
        u = 2 * TILE - 1                                       # the last tile of round 1; x = the first tile of round 2
        _add(Case("late-next-round-h%d" % half, "G", qs, _g_stream({**fill, u: {0: "plant"}, 2 * TILE: {63: "five"}}, 200), G_NBEST, 200 * TILE - 20,
                  reg, {"late": "next-round", "half": half, "u": u, "x": 2 * TILE, "filler_root": root}))
    # ---- the mirror: the heap holds NINE and NINE2 (T = 10), tiles 67 .. 73 hold references of 5 mismatches and are in flight when tile 66 admits
    # ZERO and ONE: T falls to 2 and their ballots come out empty
    lay = {0: {0: "nine", 1: "nine2"}, 66: {3: "zero", 4: "one"}}
    for t in range(67, 74):
        lay[t] = {t - 60: "five"}
    _add(Case("fall-inflight", "G", qs, _g_stream(lay, 130), G_NBEST, 130 * TILE - 20, ["replay2", "lean", "replay2-res", "replay3-h32", "replay3-h16", "replay3-h8"],
              {"fall": True, "u": 66, "x": list(range(67, 74)), "filler_root": root}))


# ---------------------------------------------------------------------------------------------------------------------------- H
# 64 columns, the probe is the root.  Every reference has the same two mismatches and 12 - c columns of N (class c = 0 .. 12: key 0 = 50 + c), so
# the tolerance never moves, every reference passes the gate and two references of one class tie on all six keys.  3 x nbest references:
# the first nbest fill the heap, the classes of the others climb slowly with a seeded jitter, so that most of them replace the root and come
# to rest at every depth, next to entries of their own class.  (nbest 1 and 2 are heaps of two: six references, and no pair of children to tie.)
H_NCHAR = 64
H_NBEST = (1, 2, 3, 4, 7, 8, 63, 64, 127, 128, 129)
H_CLASSES = 13


H_SEED = {3: 2, 4: 0, 7: 1, 8: 1, 63: 0, 64: 4, 127: 3, 128: 1, 129: 4}      # the first seed whose stream reaches every depth (test_replay_edges_cpu)


def h_classes(nbest):
    if nbest <= 2:                                                # a heap of two (src/min_heap.c:58): down one level, stay the root, twice more
        return [0, 0, 1, 1, 2, 2]
    rng = np.random.default_rng(H_SEED[nbest])
    first = rng.integers(0, 4, size=nbest)
    base = np.floor(np.arange(2 * nbest) * 8 / (2 * nbest)).astype(int)
    cl = np.concatenate([first, np.clip(base + rng.integers(0, 5, size=2 * nbest), 0, H_CLASSES - 1)])
    return [int(c) for c in cl]


def _h_cases():
    root = make_root(H_NCHAR, 303)
    qs = [root] + [edit(root, subs=c) for c in ((20, 21), (22, 23))]
    for nb in H_NBEST:
        cl = h_classes(nb)
        refs = rows([edit(root, subs=(0, 1), to_n=range(64 - (H_CLASSES - 1 - c), 64)) for c in cl])
        regs = ["replay3", "replay2", "replay2-acgt", "wide"] + (["lean"] if nb <= MC_LIMIT and nb in (3, 8, 63, 127) else []) + (["replay2-q256"] if nb > MC_LIMIT else [])
        _add(Case("nbest%d" % nb, "H", qs, refs, nb, len(refs), regs, {"classes": cl}))


# ---------------------------------------------------------------------------------------------------------------------------- K
# 128 columns.  The probe is the root with N at column 10 and R at column 11 (column 12 holds A); a second query differs from the root at
# columns 20, 21, 22, which are therefore polymorphic, and holds N at column 13.  A rung is one tile: k copies of A (they evict whatever the heap held: every rung has
# four N fewer than the one before, so it is far ahead on key 0 -- and the worst kept entry is then A), then B at the next lane.  A's
# mismatches: columns 30, 31, 32 and Y against the probe's R, so T = 5 throughout.
K_NCHAR = 128
K_N, K_R, K_A = 10, 11, 12
K_POLY = (20, 21, 22)
K_MIS = (30, 31, 32)
K_NZONE = 40                                                      # A of rung r holds N in columns 40 .. 40 + 4 (K_RUNGS - r) + 3
K_FREE = 120                                                      # a matching column outside every zone
# rung: (name, key that differs, +1 | -1 | 0, what A carries beyond the default, what B changes in A, enters)
K_LADDER = (
    ("key0-up", 0, +1, {}, {"match": K_NZONE}, True),
    ("key0-down", 0, -1, {}, {"n": K_FREE}, False),
    ("key1-up", 1, +1, {}, {"put": (K_R, "R")}, True),
    ("key1-down", 1, -1, {"put": (K_R, "R")}, {"put": (K_R, "Y")}, False),
    ("key2-up", 2, +1, {"put": (K_A, "Y"), "match": K_MIS[2]}, {"put": (K_A, "R")}, True),          # (A keeps four mismatches)
    ("key2-down", 2, -1, {"put": (K_A, "R"), "match": K_MIS[2]}, {"put": (K_A, "Y")}, False),
    ("key3-up-at-the-gate", 3, +1, {}, {"mis": K_NZONE}, False),       # one more valid pair with the same matches: m == T, the gate refuses
    ("key3-down", 3, -1, {}, {"n": K_MIS[0]}, False),
    ("key4-up", 4, +1, {"mis": K_POLY[0], "match": K_MIS[0]}, {"match": K_POLY[0], "mis": K_MIS[0]}, True),
    ("key4-down", 4, -1, {}, {"mis": K_POLY[0], "match": K_MIS[0]}, False),
    ("key5-up", 5, +1, {"n": K_N}, {"match": K_N}, True),
    ("key5-down", 5, -1, {}, {"n": K_N}, False),
    ("equal", None, 0, {}, {}, False),
    ("key0-up2-at-the-gate", 0, +2, {}, {"match": (K_NZONE, K_NZONE + 1), "mis": K_NZONE + 2}, False),   # ahead on key 0 with m == T
    ("key0-up2-inside", 0, +2, {}, {"match": (K_NZONE, K_NZONE + 1)}, True),                               # m == T - 1
)
# --acgt (assemble_scores<true>): key 0 = matches, key 1 = pairs of two ACGT, key 2 = matches outside the constant-and-complete columns, key 3 = the
# reference's valid sites, key 4 = mismatches outside the polymorphic columns, key 5 = mismatches on them.  Keys 4 and 5 add up to key 1 - key 0, so
# two references that tie on keys 0 .. 4 tie on key 5: the ladder ends at key 4.  Column 13 holds N in the second query (not polymorphic, not constant
# and complete).  A's mismatches: columns 30, 31, 32 (Y against R is no pair here), T = 4.
K_M = 13
K_LADDER_ACGT = (
    ("key0-up", 0, +1, {}, {"match": K_NZONE}, True),
    ("key0-down", 0, -1, {}, {"n": K_FREE}, False),
    ("key1-up-at-the-gate", 1, +1, {}, {"mis": K_NZONE}, False),
    ("key1-down", 1, -1, {}, {"n": K_MIS[0]}, False),
    ("key2-up", 2, +1, {"mis": K_POLY[0], "match": K_MIS[0]}, {"match": K_POLY[0], "mis": K_MIS[0]}, True),
    ("key2-down", 2, -1, {}, {"mis": K_POLY[0], "match": K_MIS[0]}, False),
    ("key3-up", 3, +1, {"n": K_N}, {"match": K_N}, True),
    ("key3-down", 3, -1, {}, {"n": K_N}, False),
    ("key4-up", 4, +1, {"mis": K_POLY[0], "match": K_MIS[0]}, {"match": K_POLY[0], "mis": K_M}, True),     # a mismatch moves off the polymorphic columns: key 5 falls by one
    ("key4-down", 4, -1, {"mis": K_M, "match": K_MIS[0]}, {"match": K_M, "mis": K_POLY[0]}, False),
    ("equal", None, 0, {}, {}, False),
    ("key0-up2-at-the-gate", 0, +2, {}, {"match": (K_NZONE, K_NZONE + 1), "mis": K_NZONE + 2}, False),
    ("key0-up2-inside", 0, +2, {}, {"match": (K_NZONE, K_NZONE + 1)}, True),
)
K_LADDERS = {"default": K_LADDER, "acgt": K_LADDER_ACGT}
K_LANE = 7


def _k_apply(root, a, ch):
    a = np.array(a, dtype=np.uint8)
    for what, v in ch.items():
        if what == "put":
            a[v[0]] = ord(v[1])
            continue
        for c in (v if isinstance(v, tuple) else (v,)):
            a[c] = root[c] if what == "match" else ord("N") if what == "n" else _ROT[root[c]]
    return a


def k_pair(root, r, ladder="default"):
    _name, _j, _d, a_ch, b_ch, _e = K_LADDERS[ladder][r]
    base = edit(root, subs=K_MIS, to_n=range(K_NZONE, K_NZONE + 4 * (len(K_LADDER) - r) + 4), put={K_R: "Y"})
    a = _k_apply(root, base, a_ch)
    return a, _k_apply(root, a, b_ch)


def k_positions(nbest, ladder="default"):
    """per rung: (ordinals of the copies of A, ordinal of B)"""
    k = max(2, nbest)
    return [(list(range(r * TILE + K_LANE, r * TILE + K_LANE + k)), r * TILE + K_LANE + k) for r in range(len(K_LADDERS[ladder]))]


def _k_cases():
    root = make_root(K_NCHAR, 404)
    root[K_A] = ord("A")
    probe = edit(root, put={K_N: "N", K_R: "R"})
    qs = [probe, edit(root, subs=K_POLY, to_n=(K_M,))]
    regs = {"default": ["replay3", "replay3-h8", "replay2", "replay2-res", "replay2-acgt", "lean", "wide"], "acgt": ["replay2-acgt", "replay2-acgt-res", "wide-acgt", "replay2"]}
    for ladder in ("default", "acgt"):
        for nb in (1, 3):
            n = len(K_LADDERS[ladder]) * TILE - 11
            a = far_rows(root, n, 45, 4000 + nb, cols=np.r_[0:K_NZONE, 111:K_NCHAR])
            a[:, K_NZONE:111] = ord("N")                          # (key 0 below every A's: before the first rung they fill the heap and A evicts them)
            for r, (ia, ib) in enumerate(k_positions(nb, ladder)):
                ra, rb = k_pair(root, r, ladder)
                a[ia] = ra
                a[ib] = rb
            _add(Case("%snbest%d" % ("" if ladder == "default" else "acgt-ladder-", nb), "K", qs, rows(a), nb, n, regs[ladder], {"root": root, "filler_root": root, "ladder": ladder}))


# ---------------------------------------------------------------------------------------------------------------------------- T
# 128 columns, heaps of 2 (nbest 1, src/min_heap.c:58).  Two first references with t = T - 1 mismatches and twenty N fix the tolerance.  Tile 2
# holds E (t mismatches, one N fewer: ahead on key 0, enters) and G (t + 1 = T mismatches, no N: ahead on key 0, refused by the gate); tile 3 holds
# X, whose mismatch count is the next threshold above t (t + 5 past the last one): counted by the coarser bound, refused by the gate.
# `cons`: the probe alone and clean, every column constant and complete (CONS = true).  `gappy`: the probe has N in the last 32 columns and a
# second query in the first 96 (n_idx_c == 0, CONS = false).  All mismatches lie in the first 96 columns.
T_NCHAR, T_COLS = 128, 96
T_VALUES = (0, 1, 2, 3, 4, 5, 6, 8, 9, 14, 15, 16)              # T - 1: each threshold and the count after it


def t_layout(t):
    nxt = [x for x in TB8_THR if x > t]
    return {"A": 0, "B": 1, "E": 2 * TILE + 5, "G": 2 * TILE + 9, "X": 3 * TILE, "x_mis": nxt[0] if nxt else t + 5}


def _t_cases():
    root = make_root(T_NCHAR, 505)
    sets = {"cons": [root], "gappy": [edit(root, to_n=range(T_COLS, T_NCHAR)), edit(root, to_n=range(T_COLS))]}
    for t in T_VALUES:
        lay = t_layout(t)
        n = 3 * TILE + 30
        a = far_rows(root, n, 40, 5000 + t, cols=np.arange(T_COLS))
        a[lay["A"]] = edit(root, subs=range(t), to_n=range(60, 80))
        a[lay["B"]] = edit(root, subs=range(1, t + 1), to_n=range(60, 80))
        a[lay["E"]] = edit(root, subs=range(2, t + 2), to_n=range(60, 79))
        a[lay["G"]] = edit(root, subs=range(3, t + 4))
        a[lay["X"]] = edit(root, subs=range(4, 4 + lay["x_mis"]))
        for name, qs in sets.items():
            _add(Case("%s-t%d" % (name, t), "T", qs, rows(a), 1, n, ["replay3", "replay3-h8", "replay2"] + (["wide"] if t in (4, 15) else []),
                      dict(lay, t=t, cons=name == "cons", filler_root=root)))


# ---------------------------------------------------------------------------------------------------------------------------- S
# 416 columns = 13 words of 32.  A sequence `lists` a word when the word holds a partially ambiguous code (R here).  The probe lists its
# first n_q words (R at the word's column 3, where the root is set to A: a reference's A there is a partial match); a reference lists n_r
# words: the LAST n_r words (R at column 5 of the word, root A: a partial match against the probe's A; the lists meet only when n_q + n_r exceeds the 13
# words, and then in other columns of the word), or `shared` = the FIRST n_r words (R at column 3, under the probe's own R: a text match; and at column 5).  The references climb on key 0 (4 N fewer each), so each is
# compared exactly and enters.
S_NCHAR, S_WORDS = 416, 13
S_COUNTS = (0, 1, 10, 11, 12)
S_QCOL, S_RCOL = 3, 5
S_CUT_R = (35, 67)                                                # the columns of R in the probe of `cut-listed`


S_BAD = 30                                                        # valid sites without an ACGT match of every climbing reference (S[3] - S[0])


def s_ref(root, probe, level, n_r, shared):
    words = range(n_r) if shared else range(S_WORDS - n_r, S_WORDS)
    put = {}
    for w in words:
        put[32 * w + S_RCOL] = "R"
        if shared:
            put[32 * w + S_QCOL] = "R"
    # mismatches and N in columns 8 .. 31 of the words: clear of the columns above
    free = [32 * w + c for c in range(8, 32) for w in range(S_WORDS)]
    a = edit(root, put=put)
    acgt = np.isin(a, np.frombuffer(b"ACGT", dtype=np.uint8))
    bad = int((~(acgt & (a == probe))).sum())                     # R against A, R against R, A against the probe's R: valid, no ACGT match
    n_sub = S_BAD - bad
    assert n_sub >= 0
    return edit(a, subs=free[:n_sub], to_n=free[n_sub:n_sub + 4 * (40 - level)])


def s_stream(n_q, overflow):
    """references in stream order with (n_r, shared); overflow: the ones that list AMB_CAP + 1 words"""
    kinds = []
    for n_r in ((12,) if overflow else (0, 1, 10, 11)):
        kinds += [(n_r, False), (n_r, True)]
    kinds = [k for k in kinds if not (k[1] and (k[0] == 0 or n_q == 0))] or [(0, False)]
    return kinds


def _s_cases():
    root = make_root(S_NCHAR, 606)
    for w in range(S_WORDS):
        root[32 * w + S_QCOL] = ord("A")
        root[32 * w + S_RCOL] = ord("A")
    for n_q in S_COUNTS:
        probe = edit(root, put={32 * w + S_QCOL: "R" for w in range(n_q)})
        for overflow in (False, True):
            kinds = s_stream(n_q, overflow)
            n = TILE + 20
            a = far_rows(root, n, 60, 6000 + n_q, cols=np.array([32 * w + c for w in range(S_WORDS) for c in range(8, 32)]))
            at = ([0, 1] + [4 + 5 * i for i in range(len(kinds))])[:len(kinds)] + [TILE + 3 + 2 * i for i in range(len(kinds))]   # each kind twice: in both tiles; the first two fill the heap
            for lvl, (o, (n_r, shared)) in enumerate(zip(at, kinds + kinds)):
                a[o] = s_ref(root, probe, lvl, n_r, shared)
            for pool in (2, 64):
                _add(Case("q%d-%s-pool%d" % (n_q, "overflow" if overflow else "listed", pool), "S", [probe], rows(a), 2, pool, ["replay3", "replay2"],
                          {"n_q": n_q, "dense": overflow or n_q > AMB_CAP, "at": at, "kinds": kinds + kinds, "root": root}))
    # ---- pairs cut at the batch snapshot: the clean probe alone (every column constant and complete), pools of 64.  Pool 0 leaves LOW (2 mismatches,
    # key 0 = 36: the root, T = 3) and NINE in the heap, so pool 1 starts with the snapshot 3.  Its plant evicts LOW: T = 10.  Then, in the same tile:
    # FIVE-LATE (5 mismatches in the last columns: the pre-score cut at 3 mismatches has counted nearly every match, its cut scores win), FIVE-EARLY (5
    # mismatches in the first columns: cut after a handful of matches, its upper-bound key 0 passes `K0 >= W[0]`, its cut scores lose), next to uncut pairs.
    # `cut-listed`: the same with a probe that lists words 1 and 2 (R at columns 35 and 67, root A) and references that list word 1 (R at column 35, under the
    # probe's R: a text match; and at column 37, against A: a partial match).  A cut pair is a slow pair of replay3_kernel: its two differences come from
    # wave_iupac_finish, where the word both sides list must be counted once (`qlisted`).  The uncut pairs behind FIVE-LATE are copies
    # of LOW here, so that it stays in the heap to the end.
    clean = make_root(128, 707)
    clean[[S_CUT_R[0], S_CUT_R[0] + 2, S_CUT_R[1]]] = ord("A")
    lay = {0: "low", 1: "nine", TILE + 4: "plant", TILE + 9: "five-early", TILE + 20: "five-late", TILE + 30: "two", TILE + 41: "five-early", TILE + 50: "one"}
    for variant in ("cut", "cut-listed"):
        put = {S_CUT_R[0]: "R", S_CUT_R[0] + 2: "R"} if variant == "cut-listed" else {}
        probe = edit(clean, put={c: "R" for c in S_CUT_R}) if variant == "cut-listed" else clean
        kinds = {"low": edit(clean, subs=(100, 101), to_n=range(2, 30), put=put), "nine": edit(clean, subs=range(100, 109), put=put), "plant": edit(clean, subs=(64,), put=put),
                 "five-early": edit(clean, subs=range(0, 5), put=put), "five-late": edit(clean, subs=range(123, 128), put=put), "two": edit(clean, subs=(70, 71), put=put),
                 "one": edit(clean, subs=(80,), put=put)}
        kinds["low"][38:100] = ord("N")
        if put:                                                   # nothing better behind FIVE-LATE: it stays in the heap with the scores the slow path gave it
            lay = {o: ("low" if k in ("two", "one") else k) for o, k in lay.items()}
        for pool in (2, 64):
            n = 2 * TILE + 9
            a = far_rows(clean, n, 50, 7000)
            for o, kname in lay.items():
                a[o] = kinds[kname]
            _add(Case("%s-pool%d" % (variant, pool), "S", [probe], rows(a), 2, pool, ["replay3", "replay3-h8", "replay2", "replay2-acgt", "wide"], {"cut": lay, "dense": False, "listed": bool(put)}))


# ---------------------------------------------------------------------------------------------------------------------------- F
# Ordinals: 130 references (two tiles and two lanes) whose mismatch counts fall and rise so that entries come from every tile; the ordinal of
# the first is 2^31 - 3, 2^32 - 3 (the low word wraps at lane 3 of the first tile) or 2^40.
F_ORDINALS = (2 ** 31 - 3, 2 ** 32 - 3, 2 ** 40)
F_N = 130
F_RANGE = (40, 100)                                               # search_resident_pool(first, n): both ends inside a tile ...
F_DB = 200                                                        # ... of a database of 200 references (the per-pool search needs the default scan: not the wide one)
F_NQ_MANY = 70


def _f_stream(root, seed, n=F_N):
    """mismatch counts that fall along the stream (with a jitter), and two copies of the root early on: the heaps end with entries of the
    first tile and of the last"""
    rng = np.random.default_rng(seed)
    a = np.tile(root, (n, 1))
    for o in range(n):
        m = max(1, 12 - o * 12 // n + int(rng.integers(0, 3)))
        a[o] = edit(root, subs=rng.choice(len(root), m, replace=False))
    a[1] = root
    a[5] = root
    return a


def _f_long(nchar, nq):
    """nq queries (the probe clean), 130 references among them a copy of the probe, an all-N row, an all-gap row and one that differs everywhere"""
    root = make_root(nchar, 808)
    qs = [root] + [edit(root, subs=(97 * i + 5, 89 * i + 4000, nchar - 1 - i)) for i in range(1, nq)]
    rng = np.random.default_rng(809)
    a = np.tile(root, (F_N, 1))
    for o in range(F_N):
        c = rng.choice(nchar, int(rng.integers(1, 40)), replace=False)
        a[o, c] = _ROT[a[o, c]]
    a[17] = root
    a[64] = ord("N")
    a[65] = ord("-")
    a[66] = _ROT[root]
    a[129] = edit(root, subs=(0, nchar - 1))
    return qs, rows(a)


def _f_cases():
    root = make_root(96, 808)
    qs = [root] + [edit(root, subs=c) for c in ((20, 21), (22, 23))]
    refs = rows(_f_stream(root, 8080))
    four = ["replay3", "replay3-res-h32", "replay2", "replay2-res", "replay2-acgt", "replay2-acgt-res", "lean", "wide", "wide-res"]
    for o0 in F_ORDINALS:
        _add(Case("ordinal%d" % o0, "F", qs, refs, 5, F_N, four, {"ordinal0": o0}))
    _add(Case("pool-cut-both-ends", "F", qs, rows(_f_stream(root, 8081, F_DB)), 5, F_RANGE[1], ["replay3-res-h32", "replay3-res-h8", "replay2-acgt-res", "replay2-res"], {"range": F_RANGE}))
    for nchar in (WIDE_ABOVE, WIDE_ABOVE + 1):
        for nq in (1, F_NQ_MANY):
            def mk(nchar=nchar, nq=nq):
                return _f_long(nchar, nq)
            lz = _Lazy(mk)
            _add(Case("nchar%d-q%d" % (nchar, nq), "F", _LazyList(lambda lz=lz: lz.get()[0]), _LazyList(lambda lz=lz: lz.get()[1]), 5, F_N,
                      ["auto", "auto-acgt"], {"nchar": nchar, "wide": nchar > WIDE_ABOVE}))


# ---------------------------------------------------------------------------------------------------------------------------- C
# The cut of the consensus pre-score.  Heaps of C_NBEST.  Pool 0 is C_NBEST `lows` -- references with a few valid sites on idx_c and N everywhere else --
# and nothing that enters after them: ROOT1 (one match, snap1 - 1 mismatches: the worst kept entry, T = snap1, the snapshot of pool 1), n1 - 1 lows of two
# matches and snap1 + C_BIG mismatches, ROOT2 (three matches, snap2 - 1 mismatches) and lows of four matches and snap2 + C_BIG mismatches.  In pool 1 an EARLY
# plant (fewer than snap1 mismatches) evicts ROOT1: T = snap1 + C_BIG + 1.  The plants follow: each is cut at snap1, passes the gate with exactly snap1
# mismatches, keeps at least C_KEY0_MIN matches in front of its cut and so evicts one low of two matches.  Pool 1 holds n1 admissions, so its last one
# leaves ROOT2 at the root: T = snap2, the snapshot of pool 2, where the same happens with snap2.  Fewer than C_NBEST references enter, so every plant is in
# the final heap with its cut scores.  Every other reference of pools 1 and 2 is a decoy: the pool's snapshot of mismatches on the FIRST columns of idx_c (cut
# with no match at all: it passes the gate and loses on key 0; uncut it would win), thirty more anywhere and N on the columns outside idx_c.
# Query sets: `single` the clean probe alone (idx_c is every column); `trim` the same under trim = C_TRIM; `three` the probe, a query that differs from it on
# the whole word C_OUT_WORD and on six more columns, and one that differs on 24 others and holds N at three (trim = C_TRIM: idx_c is a proper subset with
# a whole word outside it; the plants have dozens of mismatches against the two other queries, whose tolerances stay at snap1, below the snapshot of pool 2);
# `two` the probe and a query that differs from it at three columns, where ROOT1 holds that query's letters: its heap starts pool 1 with the tolerance
# snap1 - 1, the snapshot is snap1 and no plant passes its gate.
C_NBEST, C_KEY0_MIN, C_BIG, C_TRIM, C_OUT_WORD = 60, 5, 8, 40, 5
C_SNAPS = (1, 2, 3, 40)
C_GEOMETRIES = {2048: (64, 1, 64), 2049: (68, 2, 34), 4096: (128, 2, 64), 4200: (132, 3, 44)}      # columns: (NW, B, lanes that hold words) -- lane_split
C_POOLS = (TILE, 2 * TILE + 9)
C_PUSH = ["replay3", "replay3-h8", "replay2", "replay2-acgt", "wide", "wide-acgt"]
C_RESIDENT = ["replay3-res-h32", "replay2-acgt-res"]
# (columns, query set, snapshots of pools 1 and 2, pool): with more than one query the snapshot is the largest tolerance, so it cannot fall
C_LIST = ((2048, "single", (2, 40), 0), (2048, "three", (1, 3), 1), (2049, "single", (3, 1), 1), (2049, "three", (2, 40), 0), (4096, "single", (40, 3), 1),
          (4096, "three", (1, 2), 0), (4200, "single", (40, 1), 0), (4200, "three", (2, 3), 1), (4200, "two", (3,), 0), (2048, "trim", (3,), 0))


def c_queries(nchar, kind, seed):
    """(root, queries, trim): queries[0] is the probe, equal to the root"""
    root = make_root(nchar, seed)
    if kind in ("single", "trim"):
        return root, [root], C_TRIM if kind == "trim" else 0
    if kind == "two":
        return root, [root, edit(root, subs=[32 * w + 5 for w in (7, 15, 23)])], 0
    p1 = list(range(32 * C_OUT_WORD, 32 * C_OUT_WORD + 32)) + [32 * w + 5 for w in (9, 17, 25, 33, 41, 49)]
    p2 = [32 * w + b for w in range(10, 58, 4) for b in (11, 19)]
    return root, [root, edit(root, subs=p1), edit(root, subs=p2, to_n=[32 * w + 13 for w in (11, 27, 43)])], C_TRIM


def c_idx_c(queries, trim):
    """the constant-and-complete columns of src/fastaseq.c:732-777 for queries of A, C, G, T and N (the CPU test: equal to the oracle's idx_c)"""
    q = np.array(queries, dtype=np.uint8)
    ok = _IS_ACGT[q].all(axis=0) & (q == q[0]).all(axis=0)
    ok[:trim] = False
    ok[q.shape[1] - trim:] = False
    return np.nonzero(ok)[0]


def c_tags(cw, row, root, ic, snap, nchar):
    """what a cut plant reaches, from cut_walk (default mode, W4 given) and the row itself: the names the coverage lists use"""
    _W4, _NW, B, _lanes = lane_split(nchar)
    row, root = _as_u8(row), _as_u8(root)
    tags = {"snap%d" % snap, "bit%d" % cw.bit if cw.bit in (0, 31) else "bit-inside", "pos-" + cw.pos, "lane%d" % cw.lane}
    if cw.pos == "only":
        tags |= {"pos-first", "pos-last"}
    if cw.lane == (int(ic[-1]) // 32) // B:
        tags.add("lane-of-the-last-site")
    if cw.col == int(ic[-1]):
        tags.add("last-column")
    if cw.mis_before >= 1:
        tags.add("nth>1")
    if cw.mis_after >= 1 and cw.match_after >= 1:
        tags.add("behind")
    front = ic[ic <= cw.col]
    mis_cols = front[(row[front] != root[front]) & ~_IS_INVALID[row[front]]]            # the snap mismatches of the walk, in order
    lanes_of = (mis_cols // 32) // B
    if snap >= 2 and len(set(lanes_of.tolist())) == snap:
        tags.add("spread")
    if snap >= 2 and (cw.word % B == 0) and cw.mis_before == 0 and int(mis_cols[-2]) // 32 == cw.word - 1:
        tags.add("cross")
    if int(((row[ic] != root[ic]) & ~_IS_INVALID[row[ic]]).sum()) > snap + C_BIG:     # uncut, the pair fails the gate at every tolerance of the case
        tags.add("beyond-the-gate")
    if (_IS_INVALID[row[front]]).any():
        tags.add("n-before")
    if (row[front] == ord("R")).any():
        tags.add("r-before")
    out = np.setdiff1d(np.arange(cw.col), ic)
    if len(out) and (row[out] != root[out]).any():
        tags.add("off-before")
    if len(out) and ((out // 32) == C_OUT_WORD).sum() == 32 and cw.word > C_OUT_WORD and (mis_cols // 32 < C_OUT_WORD).any():
        tags.add("over-a-word-outside")
    return tags


def c_required_tags(nchar):
    """every item of the lists of cut positions that exists at a geometry"""
    _NW, B, lanes = C_GEOMETRIES[nchar]
    req = {"bit0", "bit31", "pos-first", "pos-last", "lane0", "lane-of-the-last-site", "last-column", "nth>1", "behind", "spread", "cross",
           "n-before", "r-before", "off-before", "over-a-word-outside", "uncut-by-one", "beyond-the-gate"} | {"snap%d" % s for s in C_SNAPS}
    if B >= 3:
        req.add("pos-inner")
    if lanes == 64:
        req.add("lane63")
    return req


def _c_plants(root, ic, snap, nchar, kind):
    """the plants of one pool: [(name, row, wanted tags)]; a plant that cannot be placed at this geometry and snapshot (too few sites or lanes in front of it for
    snap mismatches and C_KEY0_MIN matches) is left out -- test_c_covers_every_position holds the rest against c_required_tags"""
    W4, NW, B, lanes = lane_split(nchar)
    pos = {int(c): i for i, c in enumerate(ic)}
    last_lane = (int(ic[-1]) // 32) // B
    out = []

    def plant(name, col, want, lead="run", tail=True, far=False, n=0, r=False, off=(), target=True):
        if col not in pos or pos[col] < snap - 1 + n:
            return
        pt = pos[col]
        if lead == "run":
            lead_cols = [int(c) for c in ic[pt - (snap - 1):pt]]
        else:                                                       # one mismatch per lane, in the snap - 1 lanes in front of the target's
            lane = (col // 32) // B
            lead_cols = [32 * ((lane - j) * B + j % B) + 3 for j in range(snap - 1, 0, -1)]
            if lane < snap - 1 or any(c not in pos for c in lead_cols):
                return
        first = pos[lead_cols[0]] if lead_cols else pt
        cols = lead_cols + ([col] if target else [])
        if tail:
            cols += [int(ic[p]) for p in (pt + 2, pt + 5) if p < len(ic)]
        if far:                                                     # uncut the pair is beyond every tolerance of the case: only `mc_true - snap` lets it through the gate
            cols += [int(c) for c in ic[pt + 40:pt + 40 + 3 * C_BIG]]
        put = {}
        if r:
            rc = lead_cols[0] if lead_cols else col
            if root[rc] != ord("A"):
                return
            put[rc] = "R"
        row = edit(root, subs=cols + list(off), to_n=[int(c) for c in ic[first - n:first]], put=put)
        cw = cut_walk(root, ic, row, snap, False, W4)
        if target and not (cw.cut and cw.col == col and cw.counters[0] >= C_KEY0_MIN and want <= c_tags(cw, row, root, ic, snap, nchar)):
            return
        out.append((name, row, set(want) if target else {"uncut-by-one"}))

    def first_col(lo, ok):
        return next((int(c) for c in ic[ic >= lo] if ok(int(c))), -1)
    mid = max(8, min(20, last_lane - 6))                           # a lane in the middle, clear of the word outside idx_c
    plant("bit0-first-cross", 32 * mid * B, {"bit0", "pos-first"} | ({"cross"} if snap >= 2 else set()), far=True)
    plant("bit31-last", 32 * ((mid + 2) * B + B - 1) + 31, {"bit31", "pos-last"})
    if B >= 3:
        plant("inner", 32 * ((mid + 4) * B + 1) + 12, {"pos-inner", "beyond-the-gate"}, lead="lanes" if snap <= mid else "run", far=True)
    lane0 = ic[ic < 32 * B]
    plant("lane0", int(lane0[-1]) if len(lane0) >= snap + C_KEY0_MIN else -1, {"lane0"}, far=True)
    plant("last-column", int(ic[-1]), {"last-column", "lane-of-the-last-site"}, tail=False)
    if lanes == 64 and (int(ic[-1]) // 32) // B == 63:
        plant("lane63-spread", 32 * 63 * B + 9, {"lane63"} | ({"spread"} if snap >= 2 else set()), lead="lanes")
    plant("spread", 32 * (last_lane - 1) * B + 17, {"spread"} if snap >= 2 else set(), lead="lanes")
    plant("one-word", 32 * ((mid + 6) * B) + 20, {"behind", "beyond-the-gate"} | ({"nth>1"} if snap >= 2 else set()), far=True)
    plant("one-short", 32 * ((mid + 6) * B) + 20, set(), tail=False, target=False)            # the same without its last mismatch: snap - 1, not cut
    plant("n-before", 32 * ((mid + 7) * B + B - 1) + 24, {"n-before", "behind"}, n=3)
    plant("r-before", first_col(32 * (mid + 8) * B + snap, lambda c: root[int(ic[pos[c] - (snap - 1)])] == ord("A") and 2 <= c % 32 <= 26), {"r-before"}, r=True)
    if kind != "single":
        outside = np.setdiff1d(np.arange(nchar), ic)
        lo = {"three": 32 * (C_OUT_WORD + 1) + 2, "trim": 32 * 2 + 2, "two": 32 * 8 + 2}[kind]
        off = sorted(set([int(c) for c in outside[outside < lo][-2:]] + [int(outside[0])]))      # (trimmed columns, polymorphic ones)
        plant("off-before", first_col(lo, lambda c: True), {"off-before"}, off=off)
        if kind == "three":
            plant("over-a-word-outside", 32 * (C_OUT_WORD + 1), {"over-a-word-outside", "bit0"} if snap >= 2 else {"bit0"}, off=off[:1])
    return out


def _c_low(root, ic, k, m):
    """a low: k matches and m mismatches on the last columns of idx_c, N elsewhere"""
    keep = [int(c) for c in ic[len(ic) - (k + m):]]
    a = edit(root, subs=keep[k:])
    gone = np.ones(len(a), dtype=bool)
    gone[keep] = False
    a[gone] = ord("N")
    return a


def _c_build(nchar, kind, snaps, pool, seed):
    root, qs, trim = c_queries(nchar, kind, seed)
    ic = c_idx_c(qs, trim)
    sets = [_c_plants(root, ic, s, nchar, kind) for s in snaps]
    step = [max(1, (pool - 8) // max(1, len(p))) for p in sets]
    assert all(6 + st * len(p) < pool for st, p in zip(step, sets))
    n_in = [1 + len(p) for p in sets]                              # admissions of pools 1 and 2: the EARLY plant and every plant
    assert sum(n_in) + 2 <= C_NBEST <= pool
    # ---- pool 0: the lows, worst first; then references without a match, which do not enter
    lows = [_c_low(root, ic, 2, snaps[0] + C_BIG) for _ in range(n_in[0] - 1)]
    root1 = _c_low(root, ic, 1, snaps[0] - 1)
    if kind == "two":                                              # one of ROOT1's mismatches moves to a column where it holds the other query's letter
        root1 = _c_low(root, ic, 1, snaps[0] - 2)
        root1[32 * 7 + 5] = qs[1][32 * 7 + 5]
    if len(snaps) == 2:
        lows += [_c_low(root, ic, 3, snaps[1] - 1)] + [_c_low(root, ic, 4, snaps[1] + C_BIG) for _ in range(C_NBEST - n_in[0] - 1)]
    else:
        lows += [_c_low(root, ic, 2, snaps[0] + C_BIG) for _ in range(C_NBEST - n_in[0])]
    refs = lows + [root1] + [_c_low(root, ic, 0, max(snaps) + 2 * C_BIG) for _ in range(pool - C_NBEST)]
    plants = {}
    for p, (s, plist) in enumerate(zip(snaps, sets), start=1):
        n_here = pool if p < len(snaps) else pool - 5                # the last pool ends inside a tile
        block = far_rows(root, n_here, 30, seed + 10 * p)
        block[:, ic[:s]] = _ROT[root[ic[:s]]]                        # decoys: cut with no match in front ...
        block[:, np.setdiff1d(np.arange(nchar), ic)] = ord("N")     # ... and none on the columns outside idx_c, which count for key 0 too
        block[3] = edit(root, subs=[int(c) for c in ic[-1 - max(0, s - 2):-1]])     # EARLY: s - 2 mismatches (against the probe)
        for i, (name, row, want) in enumerate(plist):
            o = 6 + step[p - 1] * i
            if pool > 2 * TILE and i == len(plist) - 1:             # the last one in the pool's short third tile
                o = 2 * TILE + 2
            block[o] = row
            plants[p * pool + o] = {"name": name, "snap": s, "want": want, "pool": p}
        refs += list(block)
    return qs, rows(refs), plants, trim


def _c_cases():
    for i, (nchar, kind, snaps, pi) in enumerate(C_LIST):
        pool = C_POOLS[pi]
        lz = _Lazy(functools.partial(_c_build, nchar, kind, snaps, pool, 900 + 10 * i))
        regs = C_PUSH + (C_RESIDENT if nchar in (2049, 4200) else [])
        _root, qs, trim = c_queries(nchar, kind, 900 + 10 * i)
        _add(Case("n%d-%s-snap%s-pool%d" % (nchar, kind, "+".join(str(s) for s in snaps), pool), "C", qs, _LazyList(lambda lz=lz: lz.get()[1]), C_NBEST, pool, regs,
                  {"ncol": nchar, "kind": kind, "snaps": snaps, "trim": trim, "plants": _Lazy(lambda lz=lz: lz.get()[2])}))


_r_cases()
_g_cases()
_h_cases()
_k_cases()
_t_cases()
_s_cases()
_f_cases()
_c_cases()
