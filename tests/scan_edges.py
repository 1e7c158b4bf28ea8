"""Inputs that take the two-counter pair scans -- scan3_kernel (kernels_scan3.inc, the production scan) and scan2_iupac_kernel / scan2_acgt_kernel
(kernels_scan2.inc) as launch_scan2 (host_launch.inc) launches them -- to the edges of their item streams, tiles, ranges and counter halves, the
plain count that judges what the kernels write, and a small model of the stream's classification (host_qtables.inc) that says which edge an
input reaches.  The model never judges a count: plain_count does, and the oracle vouches for plain_count (tests/test_scan_edges_cpu.py).
Deterministic and seeded; no GPU code here.  tests/test_scan_edges_gpu.py runs the inputs through uvaia_gpu_shard_scan, which leaves the raw
counters, bounds and the aux block in caller-owned buffers.

The edge table: which line each group is aimed at (kernels_scan3.inc unless another file is named).
  S  item stream of a group record   RECORD: `if (n_full4) {` `for (uint32_t k = 0; k < n_full4; k++, sp += 4)` `LDS_ADD(o.v[0], gg); LDS_ADD(o.v[1], gg); LDS_ADD(o.v[2], gg); LDS_ADD(o.v[3], gg);`
                                     `for (uint32_t k = 0; k < n_gen; k += 2, ip += 24) {` `if (k + 1 < n_gen) {`  WORD_ITEMS: `for (; k >= 2; k -= 2) {` `if (k) {` `it = nx;`
                                     WORD_ITEM: `if (cur.v[3]) {` `if (h.v[0] & 1u) {`   host_qtables.inc: `const uint32_t n_full4 = (uint32_t)(full.size() + 3) / 4u;`
                                     `while (strm.size() & 3) strm.push_back((uint32_t)QS * row_b);` `else if (n_part == 0) { jsel = last_full; fm &= ~(0xFFu << (8 * last_full)); }`
                                     `const uint32_t nI = ~eqb & cls[(size_t)w * 4 + 2], nV = ~qV;`
  W  records per wave                `for (uint32_t rec = 0; rec < n_rec; rec += 2) {` `if (rec + 1 < n_rec) RECORD(PB, PA)` `const cst_u32 *sp = (const cst_u32 *)(stream + dir[2 * wave]);`
                                     `stile += stile_first;`  host_qtables.inc split4: `dir[2 * w] = (uint32_t)(base + (i0 < r.size() ? r[i0].at : end_at));` `size_t end_at = S.u.size() - 8;`
                                     host_launch.inc: `const int st_first = c->act_q0 / QS, n_st = (c->act_q1 + QS - 1) / QS - st_first;`
  P  dense polymorphic, rare columns `const size_t qstride = (size_t)NP4 * 16;` `for (int p4 = 0; p4 < NP4; p4++) {` `const int c0 = (ACGT ? te[rr] : te[rr] + NP4 * 128) - ((int)(pk & 0xFFFFu) - (int)RARE_BIAS)`
                                     RARE_ITEMS: `for (; k >= 2; k -= 2) {` `if (k) {`  RARE_ITEM: `LDS_SUB(off_, pack_acc(c_));`
                                     host_qtables.inc: `if (total - cnt[(size_t)b * 4 + major] > c->tab.rare_max) continue;` `strm.push_back((uint32_t)(c->tab.NP4 + r4) * 3072u);`
                                     `if (!real || !((qI >> b) & 1u) || ((eqb >> b) & 1u)) continue;`
  T  tiles, ranges, grid             `for (int rr = 0; rr < R; rr++) { live[rr] = trel0 + rr < n_tiles; trel[rr] = live[rr] ? trel0 + rr : trel0; }` `if (!live[rr]) continue;`
                                     `in_batch[rr] = ((int)r[rr] >= r_lo && (int)r[rr] < r_hi);`  kernels_scan2.inc scan_work_item: `group = (slot / n_qtiles) * 8 + xcd;` `return group < n_groups;`
                                     `static inline unsigned scan_grid_size(int n_qtiles, int n_groups) { return (unsigned)n_qtiles * (unsigned)((n_groups + 7) / 8) * 8u; }`
  C  counter range                   host_open.inc: `if (c->nchar > 49000) c->fullscan = true;`  uvaia_gpu.hip: `constexpr uint32_t SCAN3_BIAS = 16384u;`
                                     `if (ACGT) init[rr] = RARE_BIAS - (uint32_t)acc[rr][q];` `else init[rr] = (uint32_t)acc[rr][q] + RARE_BIAS;`
                                     host_qtables.inc: `if (c->scan_variant == 2 && (size_t)c->tab.NP4 * 128 + (size_t)c->tab.NR4 * 128 > SCAN3_BIAS - 256) c->scan_variant = 0;`
  K  packed-plane kernels            kernels_scan2.inc scan2_finish: `for (int q = wave; q < QT; q += 4) {` `const int c0 = sum4(2 * q), c1 = total - sum4(2 * q + 1);`
                                     `for (int o = 32; o > 0; o >>= 1) { m = min(m, __shfl_xor(m, o)); k = max(k, __shfl_xor(k, o)); }` `const bool in_batch = (r >= r_lo && r < r_hi);`
                                     host_launch.inc: `const int qt2 = c->qt != 8 ? 16 : c->nq <= 1 ? 1 : c->nq <= 2 ? 2 : c->nq <= 4 ? 4 : 8;`"""
import collections
import functools

import numpy as np

import oracle_lib as O

# ---- copies of the code's constants; each moves with the line it mirrors
QS = 64                      # `constexpr int QS = 64;` (host_launch.inc): queries of a super-tile of scan3_kernel
TILE = 64                    # references of a tile
SCAN3_BIAS = 16384           # `constexpr uint32_t SCAN3_BIAS = 16384u;` (uvaia_gpu.hip)
WIDE_ABOVE = 49000           # `if (c->nchar > 49000) c->fullscan = true;` (host_open.inc)
INVALID = b"NX-?O."          # what the reference calls an invalid site (src/utils.c:263)
SCAN3 = ((4, 1), (4, 2), (8, 1), (8, 2), (8, 4))      # (waves per block, reference tiles per wave) launch_scan2 can launch scan3_kernel with

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.full(256, -1, dtype=np.int8)
_CODE[_ACGT] = np.arange(4)                            # A=0 C=1 G=2 T=3: `rL[j] = B3(rC[j], rT[j], rI[j], ...)`, `rH[j] = B3(rG[j], rT[j], rI[j], ...)`
_VALID = np.ones(256, dtype=bool)
_VALID[np.frombuffer(INVALID, dtype=np.uint8)] = False
_ROT = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    _ROT[_a] = _b


def rot(a, k=1):
    """every A, C, G, T moved k letters on (A -> C -> G -> T -> A); other bytes stay"""
    a = np.asarray(a, dtype=np.uint8)
    for _ in range(k):
        a = _ROT[a]
    return a


def as_array(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)


def as_rows(a):
    return [np.asarray(r, dtype=np.uint8).tobytes() for r in a]


# ------------------------------------------------------------------------------------------------------------------ the plain count
def plain_count(qrows, refs, trim, acgt):
    """(first, second) int32 [n_query, n_ref] over the columns [trim, nchar - trim) of the raw bytes.
    default: first = #(both ACGT and equal), second = #(both valid);  --acgt: first = #(both ACGT and differ), second = #(both ACGT).
    Sums of products of 0/1 indicator rows in float64: exact for any alignment length."""
    Q, R = as_array(qrows), as_array(refs)
    lo, hi = trim, Q.shape[1] - trim
    Q, R = Q[:, lo:hi], R[:, lo:hi]
    equal = np.zeros((Q.shape[0], R.shape[0]))
    for b in _ACGT:
        equal += (Q == b).astype(np.float64) @ (R == b).astype(np.float64).T
    if acgt:
        both = (_CODE[Q] >= 0).astype(np.float64) @ (_CODE[R] >= 0).astype(np.float64).T
        return (both - equal).astype(np.int32), both.astype(np.int32)
    return equal.astype(np.int32), (_VALID[Q].astype(np.float64) @ _VALID[R].astype(np.float64).T).astype(np.int32)


def plain_valid_sites(refs):
    """the count of valid characters of each reference (whole row)"""
    return _VALID[as_array(refs)].sum(axis=1).astype(np.int32)


def plain_bounds(first, second, acgt, r0, n):
    """tmin[q][tile] over the references r0 .. r0 + n - 1 (columns of first / second are the whole database): int32 [n_query, tiles, 2] =
    (min mismatches, max key) of the tile's references inside the range, tiles counted from the one that holds r0"""
    mm, kk = (first, second - first) if acgt else (second - first, first)
    t0, t1 = r0 // TILE, (r0 + n + TILE - 1) // TILE
    out = np.zeros((first.shape[0], t1 - t0, 2), dtype=np.int32)
    for t in range(t0, t1):
        a, b = max(r0, t * TILE), min(r0 + n, (t + 1) * TILE)
        out[:, t - t0, 0] = mm[:, a:b].min(axis=1)
        out[:, t - t0, 1] = kk[:, a:b].max(axis=1)
    return out


def plain_prescore(consensus, idx_c, refs, acgt):
    """reference against consensus over idx_c: (x, second) int32 [n_ref].  default: x = ACGT matches (rt.x), second = valid (rt.w);
    --acgt: x = mismatches (rt.x), second = comparable (rt.y)"""
    idx = np.asarray(idx_c, dtype=np.int64)
    c = np.frombuffer(consensus, dtype=np.uint8)[idx]
    R = as_array(refs)[:, idx]
    both_acgt = (_CODE[c] >= 0)[None, :] & (_CODE[R] >= 0)
    if acgt:
        return (both_acgt & (R != c[None, :])).sum(axis=1).astype(np.int32), both_acgt.sum(axis=1).astype(np.int32)
    return (both_acgt & (R == c[None, :])).sum(axis=1).astype(np.int32), (_VALID[c][None, :] & _VALID[R]).sum(axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the model of the stream
def effective_rare_max(nq, rare_max):
    """`c->tab.rare_max = tn.rare_max > 0 ? tn.rare_max : tn.rare_max < 0 ? 0 : (c->nq < 64 ? 0 : std::min(64, std::max(4, c->nq / 64)));`"""
    return rare_max if rare_max > 0 else 0 if rare_max < 0 else (0 if nq < 64 else min(64, max(4, nq // 64)))


def _words(bits):
    """bool [..., 32 k] -> uint32 [..., k], bit b of a word = column 32 w + b"""
    b = bits.reshape(bits.shape[:-1] + (-1, 32)).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


Record = collections.namedtuple("Record", "g any_run full gen words")        # words: four lists of (query of the super-tile, byte mask of its full words)
RareRecord = collections.namedtuple("RareRecord", "r4 words")                # words: four lists of (query of the super-tile, sites)


class Model:
    """The classification lines of host_qtables.inc over the prepared query rows: column classes, and per super-tile of 64 queries the group
    records (who is full, general, a word or a run item in each 128-column group), the rare records and the share of each wave."""

    def __init__(self, qrows, trim, acgt, rare_max=0, nw=8, compressed=True):
        Q = as_array(qrows)
        self.nq, self.nchar = Q.shape
        self.W4 = ((self.nchar + 31) // 32 + 3) // 4                       # `c->W = (c->nchar + 31) / 32; c->W4 = (c->W + 3) / 4;`
        C = self.W4 * 128
        lo, hi = min(trim, self.nchar), max(min(trim, self.nchar), self.nchar - trim)
        inside = np.zeros(C, dtype=bool)
        inside[lo:hi] = True                                              # `pack_query_row(code_tab, q->seq[i], c->nchar, lo, hi, ...)`: nothing outside counts
        P = np.full((self.nq, C), ord("N"), dtype=np.uint8)
        P[:, :self.nchar] = Q
        code = _CODE[P]
        qI = (code >= 0) & inside
        qV = qI if acgt else (_VALID[P] & inside)                         # `return pl == 3 ? s4[2] : s4[pl];` (--acgt: the valid plane is the ACGT plane)
        cnt = np.stack([(qI & (code == b)).sum(axis=0) for b in range(4)])
        seen, poly = cnt.sum(axis=0) > 0, (cnt > 0).sum(axis=0) >= 2      # `poly |= seen & qI & ((qL ^ cL) | (qH ^ cH));`
        base = np.argmax(cnt > 0, axis=0)
        self.rare_max = effective_rare_max(self.nq, rare_max) if compressed else 0
        rare = np.zeros(C, dtype=bool)
        if self.rare_max > 0:
            major = np.argmax(cnt, axis=0)                                # `if (cnt[(size_t)b * 4 + k] > cnt[(size_t)b * 4 + major]) major = k;`
            rare = poly & (cnt.sum(axis=0) - cnt.max(axis=0) <= self.rare_max)       # `if (total - cnt[(size_t)b * 4 + major] > c->tab.rare_max) continue;`
            base = np.where(rare, major, base)
        self.dense, self.rare = poly & ~rare, rare
        self.cmask = (seen & ~poly) | rare                                # `cls[(size_t)w * 4 + 2] |= bit; cls[(size_t)w * 4 + 3] &= ~bit; rmask[(size_t)w] |= bit;`
        self.NP, self.NR = int(self.dense.sum()), int(rare.sum())
        self.NP4, self.NR4 = ((self.NP + 31) // 32 + 3) // 4, ((self.NR + 31) // 32 + 3) // 4     # `c->tab.NP4 = ((c->tab.NP + 31) / 32 + 3) / 4;`
        # `if (c->scan_variant == 2 && (size_t)c->tab.NP4 * 128 + (size_t)c->tab.NR4 * 128 > SCAN3_BIAS - 256) c->scan_variant = 0;`
        self.variant = 2 if compressed and self.NP4 * 128 + self.NR4 * 128 <= SCAN3_BIAS - 256 else 0
        eqb = qI & (code == base[None, :])                                # `const uint32_t eqb = qI & ~((qL ^ cls[...0]) | (qH ^ cls[...1]));`
        self.nI, self.nV = ~eqb & self.cmask[None, :], ~qV                # `const uint32_t nI = ~eqb & cls[(size_t)w * 4 + 2], nV = ~qV;`
        self.qI, self.eqb, self.code, self.nw = qI, eqb, code, nw
        self.n_st = (self.nq + 127) // 128 * 128 // QS                    # `const int n_st = c->nq_pad / QS;`
        self.records = [self._records(st) for st in range(self.n_st)]
        self.rare_records = [self._rare_records(st) for st in range(self.n_st)]

    def _records(self, st):
        out = []
        for g in range(self.W4):
            full, gen, words, any_run = [], [], [[], [], [], []], False
            for ql in range(QS):
                q = st * QS + ql
                if q >= self.nq:
                    break
                nI, nV = self.nI[q, g * 128:(g + 1) * 128].reshape(4, 32), self.nV[q, g * 128:(g + 1) * 128].reshape(4, 32)
                cm = self.cmask[g * 128:(g + 1) * 128].reshape(4, 32)
                if nV.all() and (nI == cm).all():                         # `full = full && nI == cls[(size_t)w * 4 + 2] && nV == 0xFFFFFFFFu;`
                    full.append(ql)
                    continue
                if not (nI.any() or nV.any()):                            # `if (!(((fx | (fx >> 16)) >> b) & 1u)) continue;`
                    continue
                n_part, part, last_full, fm = 0, 0, 0, 0
                for j in range(4):
                    if not (nI[j].any() or nV[j].any()):                  # `if (!(src[j] | src[4 + j])) continue;`
                        continue
                    if nV[j].all() and (nI[j] == cm[j]).all():            # `if (src[4 + j] == 0xFFFFFFFFu && src[j] == cls[(size_t)(g * 4 + j) * 4 + 2]) { last_full = j; fm |= 0xFFu << (8 * j); }`
                        last_full, fm = j, fm | (0xFF << (8 * j))
                    else:                                                 # `else { n_part++; part = j; }`
                        n_part, part = n_part + 1, j
                jsel = -1
                if n_part == 1:                                           # `if (n_part == 1) jsel = part;`
                    jsel = part
                elif n_part == 0:                                         # `else if (n_part == 0) { jsel = last_full; fm &= ~(0xFFu << (8 * last_full)); }`
                    jsel, fm = last_full, fm & ~(0xFF << (8 * last_full))
                if jsel >= 0:                                             # `if (jsel >= 0) { wrd[jsel].push_back(ql); wmask[ql] = fm; any_run |= fm != 0u; } else gen.push_back(ql);`
                    words[jsel].append((ql, fm))
                    any_run |= fm != 0
                else:
                    gen.append(ql)
            if full or gen or any(words):
                out.append(Record(g, any_run, full, gen, words))
        return out

    def _rare_records(self, st):
        cols = np.nonzero(self.rare)[0]
        out = []
        for r4 in range(self.NR4):
            words = [[], [], [], []]
            for j in range(4):
                kr = np.arange((r4 * 4 + j) * 32, min((r4 * 4 + j + 1) * 32, len(cols)))
                for ql in range(QS):
                    q = st * QS + ql
                    if q >= self.nq or len(kr) == 0:
                        break
                    c = cols[kr]
                    mine = self.qI[q, c] & ~self.eqb[q, c]                 # `if (!real || !((qI >> b) & 1u) || ((eqb >> b) & 1u)) continue;`
                    if mine.any():
                        words[j].append((ql, int((mine.astype(np.uint64) << (kr & 31).astype(np.uint64)).sum())))
            if any(words):                                                # `if (!(nw[0] | nw[1] | nw[2] | nw[3])) continue;`
                out.append(RareRecord(r4, words))
        return out

    @staticmethod
    def cost(rec):
        """`S.rec.push_back({hdr, 60u + 4u * n_full4 + 30u * (uint32_t)gen.size() + 14u * (uint32_t)(wrd[0].size() + ... + wrd[3].size())});`"""
        return 60 + 4 * ((len(rec.full) + 3) // 4) + 30 * len(rec.gen) + 14 * sum(len(w) for w in rec.words)

    def shares(self, costs):
        """split4: the number of records each of the nw waves takes.
        `const uint64_t goal = total * (uint64_t)(w + 1) / (uint64_t)NWs;`  `while (i < r.size() && (w == NWs - 1 || done + r[i].cost / 2 < goal)) { done += r[i].cost; i++; }`"""
        total, i, done, out = sum(costs), 0, 0, []
        for w in range(self.nw):
            i0, goal = i, total * (w + 1) // self.nw
            while i < len(costs) and (w == self.nw - 1 or done + costs[i] // 2 < goal):
                done += costs[i]
                i += 1
            out.append(i - i0)
        return out

    def record_shares(self, st):
        return self.shares([self.cost(r) for r in self.records[st]])

    def rare_shares(self, st):
        return self.shares([sum(len(w) for w in r.words) for r in self.rare_records[st]])     # `S.rare.push_back({strm.size(), nw[0] + nw[1] + nw[2] + nw[3]});`


def decode_stream(stream, sdir, n_st, nw, R):
    """query tables 7 and 8 (uint32 arrays) -> per super-tile (records, rare records, record shares, rare shares) in the model's terms"""
    row_b = 256 * R                                                       # `const uint32_t row_b = 256u * (uint32_t)c->scan_R;`
    sdir = np.asarray(sdir, dtype=np.uint32).reshape(n_st, 4 * nw)
    out = []
    for st in range(n_st):
        d = sdir[st]
        shares, rshares = [int(d[2 * w + 1]) for w in range(nw)], [int(d[2 * nw + 2 * w + 1]) for w in range(nw)]
        p, recs, rares = int(d[0]), [], []
        while True:
            h = [int(x) for x in stream[p:p + 4]]
            if h == [0, 0, 0, 4]:
                break
            n_full4, n_gen, nwords = h[1] & 0xFFFF, h[1] >> 16, [(h[2] >> (8 * j)) & 255 for j in range(4)]
            a = p + 4
            full = [int(x) // row_b for x in stream[a:a + 4 * n_full4] if int(x) != QS * row_b]
            assert all(int(x) % row_b == 0 for x in stream[a:a + 4 * n_full4])
            a += 4 * n_full4
            gen = [int(stream[a + 12 * k + 8]) // row_b for k in range(n_gen)]
            a += 12 * n_gen
            words = []
            for j in range(4):
                words.append([(int(stream[a + 4 * k + 2]) // row_b, int(stream[a + 4 * k + 3])) for k in range(nwords[j])])
                a += 4 * nwords[j]
            assert a - p == h[3], "record length"
            recs.append(Record((h[0] & ~1023) // 2048, bool(h[0] & 1), full, gen, words))
            p = a
        assert [int(x) for x in stream[p + 4:p + 8]] == [0, 0, 0, 4], "two zero headers end the group records"
        p += 8
        for _ in range(sum(rshares)):
            h = [int(x) for x in stream[p:p + 4]]
            nwords = [(h[1] >> (8 * j)) & 255 for j in range(4)]
            a, words = p + 4, []
            for j in range(4):
                words.append([(int(stream[a + 4 * k + 3]) // row_b, int(stream[a + 4 * k])) for k in range(nwords[j])])
                a += 4 * nwords[j]
            rares.append((h[0], RareRecord(-1, words)))
            p = a
        out.append((recs, rares, shares, rshares))
    return out


# ------------------------------------------------------------------------------------------------------------------ building blocks of the inputs
def make_root(nchar, seed):
    return _ACGT[np.random.default_rng(seed).integers(0, 4, nchar)]


def make_refs(root, n, seed, p_sub=0.02):
    """n references around the root: substitutions (more in later rows), N runs, sparse ambiguity codes, gaps and '?'; row 0 is the root itself"""
    rng = np.random.default_rng(seed)
    L = len(root)
    out = np.tile(np.asarray(root, dtype=np.uint8), (n, 1))
    for i in range(1, n):
        m = rng.random(L) < p_sub * rng.random() * 2
        out[i, m] = rot(out[i, m], int(rng.integers(1, 4)))
        for _ in range(int(rng.integers(0, 4))):
            a = int(rng.integers(0, L))
            out[i, a:a + int(rng.integers(1, max(2, L // 8)))] = ord("N")
        k = int(rng.integers(0, max(2, L // 300)))
        out[i, rng.integers(0, L, k)] = np.frombuffer(b"RYKMSW-?X", dtype=np.uint8)[rng.integers(0, 9, k)]
    return out


def make_queries(root, n, seed, n_poly=10):
    """n queries around the root: n_poly shared polymorphic columns, two private substitutions each, N runs in a third of them, single
    ambiguity codes and gaps in a fifth: the common stream shapes"""
    rng = np.random.default_rng(seed)
    L = len(root)
    out = np.tile(np.asarray(root, dtype=np.uint8), (n, 1))
    for c in rng.choice(L, n_poly, replace=False):
        m = rng.random(n) < 0.5
        out[m, c] = rot(out[m, c])
    for i in range(n):
        c = rng.choice(L, 2, replace=False)
        out[i, c] = rot(out[i, c], int(rng.integers(1, 4)))
        if rng.random() < 0.33:
            a = int(rng.integers(0, L))
            out[i, a:a + int(rng.integers(1, 200))] = ord("N")
        if rng.random() < 0.2:
            out[i, int(rng.integers(0, L))] = b"RY-?"[int(rng.integers(0, 4))]
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
# scans: list of (database size, [(first, n), ...]): the database is refs[:size], every range is one uvaia_gpu_shard_scan
# kernels: "scan3" = every (NW, R) of SCAN3 with scan: compressed; "scan3-R1" = the two with R = 1; "scan3-one" = (8, 2) only; "scan2" = scan: packed
# cons: (True, False) runs the case also with query->idx_c moved into idx_m (no constant-and-complete column: the CONS = false instantiations)
Case = collections.namedtuple("Case", "key group aim queries refs trim nq kernels modes scans tuning active ambig_q variant cons meta")
CASES = collections.OrderedDict()


def add(key, group, aim, queries, refs, nq=None, trim=0, kernels="scan3", modes=(False, True), scans=None, tuning=None, active=None, ambig_q=0.5, variant=None,
        cons=(True,), **meta):
    queries, refs = as_rows(queries), as_rows(refs)
    variant = (0 if kernels == "scan2" else 2) if variant is None else variant
    CASES[key] = Case(key, group, aim, queries, refs, trim, len(queries) if nq is None else nq, kernels, tuple(modes), scans or [(len(refs), [(0, len(refs))])],
                      dict(tuning or {}), active, ambig_q, variant, tuple(cons), meta)


def _col(g, off):
    return g * 128 + off


def _build_s():
    """One alignment of 3 000 columns (24 groups, the last one cut by the alignment's end) and 64 queries; groups 0 .. 20 each hold one shape."""
    root = make_root(3000, 101)
    Q = np.tile(root, (64, 1))
    rng = np.random.default_rng(102)

    def who(k, g):
        return [(7 * g + 5 * i) % 64 for i in range(k)] if k < 64 else list(range(64))

    g = 0
    want = {"full": [], "gen": [], "words": [], "runs": []}
    for k in (1, 3, 4, 5, 8, 64):                                          # S1: all-N over the whole group
        Q[who(k, g), _col(g, 0):_col(g, 128)] = ord("N")
        want["full"].append((g, k)); g += 1
    for k in (1, 2, 3, 63):                                                # S2: general items: two or three words dirty, each partly
        for n_, q in enumerate(who(k, g)):
            Q[q, _col(g, 5 + n_ % 20)] = b"N-R?"[n_ % 4]
            Q[q, _col(g, 40 + n_ % 20):_col(g, 43 + n_ % 20)] = ord("N")
            if n_ % 3 == 0:
                Q[q, _col(g, 100)] = ord("Y")
        want["gen"].append((g, k)); g += 1
    for counts in ((1, 0, 0, 0), (0, 0, 0, 1), (2, 0, 3, 0), (3, 1, 2, 5)):  # S3: word items, word by word
        qs = iter(who(sum(counts), g))
        for j, k in enumerate(counts):
            for n_ in range(k):
                Q[next(qs), _col(g, 32 * j + 3 + 5 * n_)] = b"NK-N?"[n_ % 5]
        want["words"].append((g, counts)); g += 1
    for n_full, partial in ((1, True), (2, True), (3, True), (1, False), (2, False), (3, False)):   # S4: run items
        q = who(2, g)
        a = 20 if partial else 32
        Q[q[0], _col(g, a):_col(g, 32 + 32 * n_full)] = ord("N")
        fm = sum(0xFF << (8 * j) for j in range(1, 1 + n_full))
        if not partial:
            fm &= ~(0xFF << (8 * n_full))
        if (n_full, partial) == (2, True):
            Q[q[1], _col(g, 77)] = ord("N")                                # a non-run word item in a record with a run item
        want["runs"].append((g, 0 if partial else n_full, fm)); g += 1
    q = who(6, g)                                                          # S5: all three kinds in one record
    Q[q[0:2], _col(g, 0):_col(g, 128)] = ord("N")
    Q[q[2], _col(g, 3)] = ord("N"); Q[q[2], _col(g, 64)] = ord("S"); Q[q[2], _col(g, 127)] = ord("-")
    Q[q[3], _col(g, 50)] = ord("N"); Q[q[4], _col(g, 96):_col(g, 128)] = ord("N")
    want["all3"] = g; g += 1
    # polymorphic columns inside dirty groups, some of them N in a dirty query: nI clear while nV set
    for gg, off in ((6, 45), (9, 41), (12, 3), (13, 35), (21, 7)):
        half = rng.random(64) < 0.5
        half[:2] = (True, False)
        keep = Q[:, _col(gg, off)] == root[_col(gg, off)]
        Q[half & keep, _col(gg, off)] = rot(root[_col(gg, off)])
    want["n_groups"] = g
    return root, Q, want


def _build():
    root_s, Q_s, want_s = _build_s()
    refs_s = make_refs(root_s, 130, 103)
    refs_s[5, _col(3, 0):_col(5, 0)] = ord("N")                            # a reference that is N where queries are all-N, and one with codes there
    refs_s[6, _col(0, 0):_col(21, 0):7] = ord("R")
    add("S", "S", "RECORD / WORD_ITEMS / WORD_ITEM: full lists of 1, 3, 4, 5, 8, 64; 1, 2, 3, 63 general items; word lists; run items", Q_s, refs_s, want=want_s)
    add("S-trim", "S", "`(uint32_t)QS * row_b`: the trimmed groups are all-N for all 64 queries", Q_s, refs_s, trim=130, want=want_s)

    # ---- W: records per wave
    root = make_root(1536, 201)                                            # 12 whole groups: a query without N is clean everywhere
    Q = np.tile(root, (64, 1))
    Q[3, _col(2, 17)] = ord("N"); Q[9, _col(2, 99)] = ord("N"); Q[9, _col(2, 3)] = ord("-")
    Q[11, _col(7, 0):_col(7, 128)] = ord("N")
    Q[20:40, _col(10, 64)] = ord("N")
    refs_w = make_refs(root, 130, 202)
    add("W1", "W", "exactly 3 dirty groups: with NW = 8 some waves get n_rec == 0 (`end_at`), others an odd n_rec", Q, refs_w)
    Q = np.tile(root, (128, 1))
    for i in range(64):
        Q[i, _col(i % 5, 3 * i % 128)] = ord("N")
    add("W2", "W", "`S.rec.empty()`: the second super-tile's queries are all clean", Q, refs_w)
    root = make_root(1100, 203)
    refs_g = make_refs(root, 320, 204)
    for n in (33, 64, 65, 130):
        add("W3-%d" % n, "W", "`const int n_st = c->nq_pad / QS;`: %d queries" % n, make_queries(root, n, 205 + n), refs_g[:130])
    add("W4", "W", "`stile += stile_first;` set_active_queries(64, 128)", make_queries(root, 130, 205 + 130), refs_g[:130], active=(64, 128))

    # ---- P: dense polymorphic and rare columns
    Q = np.tile(root, (64, 1))
    rng = np.random.default_rng(301)
    for i in range(64):
        Q[i, rng.choice(1100, 3)] = ord("N")
    Q[5, 300:500] = ord("N")
    add("P1", "P", "`const size_t qstride = (size_t)NP4 * 16;` NP = 0: no dense loop", Q, refs_g[:130], tuning={"rare_max": -1}, NP=0, NR=0)
    for NP in (1, 128, 129):
        Qp = Q.copy()
        for c in np.sort(rng.choice(1100, NP, replace=False)):
            m = np.arange(64) % 3 == int(rng.integers(0, 3))
            m &= Qp[:, c] == root[c]
            Qp[m, c] = rot(root[c], int(rng.integers(1, 4)))
        add("P2-%d" % NP, "P", "`te[rr] + NP4 * 128`: %d dense columns, the rest of the last group is padding" % NP, Qp, refs_g[:130], tuning={"rare_max": -1}, NP=NP, NR=0)
    Qr = Q.copy()
    for c in np.sort(rng.choice(1100, 40, replace=False)):
        who = rng.choice(64, int(rng.integers(1, 3)), replace=False)
        Qr[who, c] = rot(root[c], int(rng.integers(1, 4)))
    add("P3-rare", "P", "every polymorphic column is rare: NP4 = 0, NR4 > 0", Qr, refs_g[:130], tuning={"rare_max": 2}, NP=0, NR=40)
    add("P3-dense", "P", "rare_max: -1: the same columns dense, NR4 = 0", Qr, refs_g[:130], tuning={"rare_max": -1}, NP=40, NR=0)
    # P4 / P5 / P6: 384 rare columns (three rare groups) and a dense group, 128 queries in two super-tiles
    root = make_root(2048, 302)
    Q = np.tile(root, (128, 1))
    for i in range(64):
        Q[i, 2040 + i % 8] = ord("N")                                      # fewer valid sites: these are the first super-tile after the reordering
    rcols = 5 * np.arange(384) + 2
    for kr, c in enumerate(rcols):
        r4, j = kr // 128, kr // 32 % 4
        if r4 == 0:
            q = 10 if j == 0 else 70                                       # first super-tile: (1, 0, 0, 0)
        elif r4 == 1:
            q = 11 if j == 3 else 71                                       # (0, 0, 0, 1)
        else:
            q = (20, 21, 30, 31, 32, 40, 50, 51, 52, 53)[(0, 2, 5, 6)[j] + kr % (2, 3, 1, 4)[j]]     # (2, 3, 1, 4)
        Q[q, c] = rot(root[c], 1 + kr % 3)
    Q[12, rcols[300]] = ord("N")                                           # P6: N at a rare column beside the minority query of that column
    for c in (1, 6, 11, 501, 1006):
        Q[::2, c] = rot(root[c])                                           # dense columns: NP4 = 1
    add("P456", "P", "RARE_ITEMS: word counts (1,0,0,0), (0,0,0,1), (2,3,1,4); `(NP4 + r4) * 3072u` with NR4 = 3; N at a rare column",
        Q, make_refs(root, 130, 303), tuning={"rare_max": 2}, NP=5, NR=384)

    # ---- T: tiles, ranges, grid
    root = make_root(1100, 203)
    Qt = make_queries(root, 64, 205 + 64)
    add("T1", "T", "`if (!live[rr]) continue;` databases of 64, 65, 191 and 320 references", Qt, refs_g, scans=[(n, [(0, n)]) for n in (64, 65, 191, 320)])
    T2 = [(0, 191), (37, 1), (37, 27), (63, 2), (64, 64), (100, 91)]
    add("T2", "T", "`in_batch[rr] = ((int)r[rr] >= r_lo && (int)r[rr] < r_hi);`", Qt, refs_g[:191], scans=[(191, T2)])
    add("T3", "T", "`group = (slot / n_qtiles) * 8 + xcd;` `return group < n_groups;`: 9 tile groups x 2 super-tiles", make_queries(root, 65, 205 + 65),
        make_refs(root, 570, 401), kernels="scan3-R1")

    # ---- C: counter range
    root = make_root(49000, 501)
    Q = np.tile(root, (8, 1))
    Q[0, :] = ord("N"); Q[0, 24000:24032] = root[24000:24032]
    Q[1, 100:30000] = ord("N")
    Q[2::2, 777] = rot(root[777])
    refs_c = make_refs(root, 64, 502, p_sub=0.002)
    add("C1", "C", "the low half reaches SCAN3_BIAS + NP4 * 128 + te with te near 49 000: no carry into the valid-pair half", Q, refs_c, modes=(False,), ambig_q=1.0, NP=1)
    root = make_root(20000, 503)
    refs_c2 = make_refs(root, 64, 504, p_sub=0.002)
    for key, NP in (("C2", 126 * 128), ("C3", 126 * 128 + 1)):
        Q = np.tile(root, (6, 1))
        cols = np.arange(NP)
        Q[1::2, :NP] = rot(root[:NP])
        Q[4, cols[::50]] = root[cols[::50]]
        Q[5, 19000:19500] = ord("N")
        refs = refs_c2.copy()
        refs[1, :NP] = rot(root[:NP], 2)                                   # mismatches every query on every polymorphic column
        add(key, "C", "`(size_t)c->tab.NP4 * 128 + (size_t)c->tab.NR4 * 128 > SCAN3_BIAS - 256`: NP4 = %d" % ((NP + 127) // 128), Q, refs, modes=(True,),
            tuning={"rare_max": -1}, variant=2 if key == "C2" else 0, kernels="scan3" if key == "C2" else "scan3-one", NP=NP)

    # ---- K: the packed-plane two-counter kernels
    root = make_root(1100, 203)
    for n in (1, 2, 3, 5, 8, 9, 17, 32):
        add("K-%d" % n, "K", "`for (int q = wave; q < QT; q += 4)` QT = %d" % (16 if n > 8 else 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8),
            make_queries(root, n, 600 + n, n_poly=4), refs_g[:191], kernels="scan2", scans=[(64, [(0, 64)]), (191, T2)], cons=(True, False))


_build()


def variants(case):
    """(acgt, (NW, R) or None, cons) of every run of a case"""
    nwr = {"scan3": SCAN3, "scan3-R1": tuple(v for v in SCAN3 if v[1] == 1), "scan3-one": ((8, 2),), "scan2": (None,)}[case.kernels]
    return [(acgt, v, cons) for acgt in case.modes for v in nwr for cons in case.cons]


def runs(group=None):
    return [(c.key, a, v, k) for c in CASES.values() if group in (None, c.group) for a, v, k in variants(c)]


def run_id(key, acgt, v, cons):
    return "%s-%s-%s%s" % (key, "acgt" if acgt else "iupac", "scan2" if v is None else "nw%dr%d" % v, "" if cons else "-nocons")


def tuning(case, v):
    t = dict(case.tuning)
    if v is None:
        t["scan"] = "packed"
    else:
        t.update({"scan": "compressed", "scan_waves_per_block": v[0], "scan_tiles_per_wave": v[1]})
    return t


@functools.lru_cache(maxsize=None)
def query(key, acgt):
    c = CASES[key]
    return O.Query(list(c.queries), ["q%d" % i for i in range(len(c.queries))], trim=c.trim, acgt=acgt, ambig_q=c.ambig_q)


@functools.lru_cache(maxsize=None)
def gold(key, acgt):
    """the plain count of the whole case: (first, second) [n_query, n_ref], valid sites [n_ref], pre-score (x, second) [n_ref] or None"""
    c, q = CASES[key], query(key, acgt)
    first, second = plain_count(q.seqs, c.refs, c.trim, acgt)
    pre = plain_prescore(q.consensus, q.idx_c, c.refs, acgt) if len(q.idx_c) else None
    return first, second, plain_valid_sites(c.refs), pre


@functools.lru_cache(maxsize=None)
def model(key, acgt, nw=8):
    c, q = CASES[key], query(key, acgt)
    return Model(q.seqs, c.trim, acgt, rare_max=c.tuning.get("rare_max", 0), nw=nw, compressed=c.kernels != "scan2")


def qt2(nq):
    """`c->qt = c->nq <= 8 ? 8 : 16;`  `const int qt2 = c->qt != 8 ? 16 : c->nq <= 1 ? 1 : c->nq <= 2 ? 2 : c->nq <= 4 ? 4 : 8;`"""
    return 16 if nq > 8 else 1 if nq <= 1 else 2 if nq <= 2 else 4 if nq <= 4 else 8


def written_rows(nq, variant, active=None):
    """the rows of cnt / tmin a launch covers.  scan3: `stile += stile_first;` over n_st super-tiles; scan2: QT * n_qtiles"""
    if variant == 2:
        q0, q1 = active or (0, nq)
        return (q0 // QS) * QS, ((q1 + QS - 1) // QS) * QS
    return 0, (nq + qt2(nq) - 1) // qt2(nq) * qt2(nq)
