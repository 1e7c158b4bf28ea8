"""Inputs that take the wavefront aligner (wfa_align_kernel, uvaia_amd/csrc/uvaia_align.hip) to its numeric edges -- offsets that stop
fitting 16 bits, wavefronts around the width kept in LDS and around the strides of the reduction, penalties at the edge of the header ring,
extension runs around 8 and 1 024 characters, backtrace runs around 63 -- and a model of the kernel's per-step bookkeeping (step_paths) that
shows, on the CPU, which path every step of an input takes.  The model never judges a result: the oracle does.  Deterministic and seeded; no
GPU code here.  tests/test_align_edges_cpu.py shows that every input reaches the edge it is built for and stays inside what the kernel
accepts, tests/test_align_edges_gpu.py runs the inputs on the device."""
import collections
import functools

import fixtures as F
import oracle_lib as O

# ---- copies of the kernel's constants (uvaia_amd/csrc/uvaia_align.hip); each moves with the line it mirrors
WL = 2560                   # `constexpr int WL = 2560;`  widest wavefront kept in LDS
RM, RID = 5, 2              # `constexpr int RM = 5, RID = 2;`  LDS slots of M and of I / D wavefronts
RING = 64                   # `constexpr int RING = 64;`  headers kept in LDS; penalties are below this (uvaia_align_open)
HDR_INTS = 8                # `constexpr int HDR_INTS = 8;`
HDR_PAGE_SCORES = 2048      # `constexpr int HDR_PAGE_SCORES = 2048;`
MAX_HDR_PAGES = 256         # `constexpr int MAX_HDR_PAGES = 256;`
MAX_OWN = 512               # `constexpr int MAX_OWN = 512;`  chunks a query may take from the pool
MIN_CHUNK_LOG2 = 19         # `int lg = 19;` in ensure_pool_memory
MAX_CHUNK_LOG2 = 28         # `if (lg > 28)` in ensure_pool_memory
OFFSET_LIMIT = 65535        # `const bool fits = w <= WL && tlen + step + 32 < 65535;`

WORKSPACE = 256 << 20       # what the device tests open every aligner with

DEFAULTS = dict(mismatch=4, gap_opening=6, gap_extension=2, min_wavefront_length=128, max_distance_threshold=512)   # uvaia_align_default_options


def w16_of(w):
    return (w + 15) & ~15   # `w16_of` of the kernel


def chunk_log2(plen, gap_extension):
    """the chunk size ensure_pool_memory chooses for a reference of plen sites"""
    widest = plen * 5 // 2 + 64
    lg = MIN_CHUNK_LOG2
    while (1 << lg) < (gap_extension + 2) * 2 * widest:
        lg += 1
    return lg


def gcd3(a, b, c):
    from math import gcd
    return gcd(gcd(a, b), c)


Step = collections.namedtuple("Step", "score step w fits resident mem_s mem_g mem_e lds_only id_to_memory ring_pos wraps chunks pages page_at refused")


def step_paths(shape, plen, tlen, penalties):
    """The kernel's bookkeeping, one Step per score that has a wavefront, from the oracle's per-score limits (O.wfa_shape) and penalties
    (mismatch, gap_opening, gap_extension).  mem_s / mem_g / mem_e: the step reads M of score - x / M of score - o - e / I or D of score - e
    from memory and not from LDS; chunks: taken from the pool so far (on top of the block's two); pages: header pages opened so far; page_at:
    score at which the last one was opened; refused: None, or the status the kernel would end the query with (the list ends there)."""
    x, o, e = penalties
    oe = o + e
    g = gcd3(x, oe, e)
    id_deep = e // g >= RID                                     # `const bool id_deep = P.e / P.g >= RID;`
    chunk_words = 1 << chunk_log2(plen, e)
    max_score = min(plen * x + o + 2 * plen * e, 0x3fffffff)    # `a->P.max_score` in uvaia_align_open
    hdr = {}                                                    # score -> (flags, res): what the LDS ring holds of it
    state = dict(cur_used=0, n_own=0)
    step, ring_pos, widest16, wraps, pages, page_at = 0, 0, 16, 0, 0, -1

    def take(words):                                            # the `take` lambda
        if state["cur_used"] + words > chunk_words:
            if state["n_own"] >= MAX_OWN:
                return False
            state["n_own"] += 1
            state["cur_used"] = 0
        state["cur_used"] += words
        return True

    def stop(score, why):
        return Step(score, step, 0, False, False, False, False, False, False, False, ring_pos, wraps, state["n_own"], pages, page_at, why)

    for score, lo_base, hi_base, _lo, _hi, has_i, has_d in shape:
        assert score % g == 0
        if score > max_score:                                   # `if (score > P.max_score) { status = ST_MAXSCORE; break; }`
            yield stop(score, "ST_MAXSCORE")
            return
        while pages * HDR_PAGE_SCORES <= score:                 # `if (score / HDR_PAGE_SCORES != (score - P.g) / HDR_PAGE_SCORES || score == 0)`
            if pages >= MAX_HDR_PAGES:
                yield stop(score, "ST_HDRPAGES")
                return
            page_at = -(-pages * HDR_PAGE_SCORES // g) * g      # the first score the loop visits in that page
            if not take(HDR_PAGE_SCORES * HDR_INTS):
                yield stop(score, "ST_OVERFLOW")
                return
            pages += 1
        w = hi_base - lo_base + 1
        w16 = w16_of(w)
        hist_words = w16 + w16_of((w + 3) // 4)
        fits = w <= WL and tlen + step + 32 < OFFSET_LIMIT
        src = []
        for back, slots in ((x, RM), (oe, RM), (e, RID)):
            flags, res = hdr.get(score - back, (0, 0))
            src.append((flags, res, bool(res) and step - (res - 1) < slots))
        (fs, _, lds_s), (fg, _, lds_g), (fe, _, lds_e) = src
        ex_s, ex_g, ex_e = bool(fs & 1), bool(fg & 1), bool(fe & 6)
        sources_in_lds = (not ex_s or lds_s) and (not ex_g or lds_g) and (not ex_e or lds_e)
        all_sources = score > 0 and ex_s and ex_g and (fe & 6) == 6
        lds_only = fits and all_sources and sources_in_lds and not id_deep
        if not lds_only:
            widest16 = max(widest16, w16)
            if (e + 2) * 2 * widest16 > chunk_words or hist_words > chunk_words:
                yield stop(score, "ST_TOOWIDE")
                return
            if ring_pos + 2 * w16 > chunk_words:
                ring_pos = 0
                wraps += 1
            ring_pos += 2 * w16
        if not take(hist_words):
            yield stop(score, "ST_OVERFLOW")
            return
        resident = lds_only or fits
        id_to_memory = not lds_only and (not resident or id_deep)
        yield Step(score, step, w, fits, resident, ex_s and not lds_s, ex_g and not lds_g, ex_e and not lds_e, lds_only, id_to_memory,
                   ring_pos, wraps, state["n_own"], pages, page_at, None)
        step += 1
        hdr[score] = (1 | (2 if has_i else 0) | (4 if has_d else 0), step if resident else 0)
        hdr.pop(score - RING, None)


def pool_fits(own_chunks, plen, opts):
    """whether run_passes finishes a pool whose queries take own_chunks[i] chunks in its first launch, whatever the order: the blocks it
    starts (`std::min(std::min(n_todo, a->max_blocks), a->n_chunks / 3)`) share `n_chunks - 2 * blocks` chunks"""
    max_blocks = opts.get("max_blocks", 0)
    n_chunks = opts.get("workspace_bytes", WORKSPACE) // (4 << chunk_log2(plen, penalties_of(opts)[2]))
    if n_chunks < 3:
        return False
    blocks = max(1, min(len(own_chunks), n_chunks // 3, max_blocks if max_blocks > 0 else 1 << 30))
    return sum(sorted(own_chunks)[-blocks:]) <= n_chunks - 2 * blocks


# ---- the oracle's answer to one query, kept for the tests that share it
def oracle_kw(opts):
    d = dict(DEFAULTS)
    d.update({k: v for k, v in opts.items() if k in DEFAULTS})
    return dict(penalties=(0, d["mismatch"], d["gap_opening"], d["gap_extension"]), min_wavefront_length=d["min_wavefront_length"],
                max_distance_threshold=d["max_distance_threshold"])


def penalties_of(opts):
    return oracle_kw(opts)["penalties"][1:]


@functools.lru_cache(maxsize=None)
def _expected(ref, seq, kw):
    score, cigar, cells, width = O.wfa_align(ref, seq, **dict(kw))
    return score, O.align_project(cigar, seq), cells, width, cigar if len(ref) * len(seq) <= GOTOH_CELLS else None


def expected(ref, seq, opts):
    """(score, row on the reference's columns, cells, widest wavefront, CIGAR or None for a long pair) as the oracle gives them"""
    return _expected(ref, seq, tuple(sorted(oracle_kw(opts).items())))


Paths = collections.namedtuple("Paths", "score cigar cells width shape steps")


def paths(ref, seq, opts):
    """the oracle's score, CIGAR, cells, widest wavefront and per-score limits, and the kernel's path through them (list of Step)"""
    kw = oracle_kw(opts)
    score, cigar, cells, width, shape = O.wfa_run(ref, seq, kw["penalties"], kw["min_wavefront_length"], kw["max_distance_threshold"], 1 << 30, True)
    return Paths(score, cigar, cells, width, shape, list(step_paths(shape, len(ref), len(seq), kw["penalties"][1:])))


GOTOH_CELLS = 4_000_000     # pairs up to this many cells of the full table are also scored by the Gotoh recurrence


def is_complete(opts):
    return opts.get("min_wavefront_length", DEFAULTS["min_wavefront_length"]) <= 0


Pool = collections.namedtuple("Pool", "name ref opts seqs")     # opts: options of align.Aligner (its workspace is WORKSPACE unless they say otherwise)

_STEP = bytes.maketrans(b"ACGT", b"CGTA")


def other(ch):
    """a letter that is not ch (bytes of length one or more: every site changed)"""
    return ch.translate(_STEP)


def n_run(seq, a, n):
    return seq[:a] + b"N" * n + seq[a + n:]


# ------------------------------------------------------------------------------------------------------ A: offsets and 16 bits
A_LEN = 65600
A_TL = (65400, 65502, 65503, 65535, 65536, 65600)
A_RUN, A_DEL = (20000, 150), (40000, 7)


@functools.lru_cache(maxsize=None)
def group_a():
    """ref[:tl + 7] without seven sites (so the query has tl characters; the last one has 65 593: the reference ends) and a run of 150 N;
    tl = 65 400 loses `fits` at step 103, 65 502 after step 0, the others never fit; one query longer than the reference"""
    ref = F.random_acgt(A_LEN, 20261201)
    seqs = []
    for tl in A_TL:
        q = ref[:A_DEL[0]] + ref[A_DEL[0] + A_DEL[1]:tl + A_DEL[1]]
        seqs.append(n_run(q, *A_RUN))
    seqs.append(ref + F.random_acgt(100, 20261202))
    return [Pool("A", ref, {}, tuple(seqs))]


# ------------------------------------------------------------------------------- B: widths around WL, the strides, the reduction
B_LEN = 6000
B_MIN_LEN = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2559, 2560, 2561)
B_MAX_DIST = (0, 1, 50, 512)
B_SETTINGS = [dict(min_wavefront_length=0)] + [dict(min_wavefront_length=m, max_distance_threshold=t) for m in B_MIN_LEN for t in B_MAX_DIST]


@functools.lru_cache(maxsize=None)
def b_query():
    ref = F.random_acgt(B_LEN, 20261203)
    q = n_run(ref[:4500] + ref[4507:], 2000, 1400)
    return ref, q


def group_b(setting):
    ref, q = b_query()
    return [Pool("B", ref, dict(setting), (q,))]


@functools.lru_cache(maxsize=None)
def group_b_outside():
    """the end cell's diagonal lies outside the first reduced wavefronts: a query that is the middle of the reference, and the converse"""
    ref = F.random_acgt(4000, 20261204)
    return [Pool("B-inner-query", ref, {}, (ref[700:2700],)), Pool("B-inner-reference", ref[700:2700], {}, (ref,))]


# ---------------------------------------------------------------------------------------------------------------- C: penalties
C_LEN = 1500
C_SETS = [   # (name, options, length of the N run)
    ("deep-ring-wrap", dict(mismatch=2, gap_opening=12, gap_extension=3, min_wavefront_length=0), 400),
    ("deep-ring-wrap-600", dict(mismatch=2, gap_opening=12, gap_extension=3, min_wavefront_length=0), 600),
    ("ring-edge", dict(mismatch=63, gap_opening=40, gap_extension=23), 100),
    ("ring-edge-complete", dict(mismatch=63, gap_opening=40, gap_extension=23, min_wavefront_length=0), 100),
    ("gcd5", dict(mismatch=5, gap_opening=5, gap_extension=5), 850),
    ("gcd5-complete", dict(mismatch=5, gap_opening=5, gap_extension=5, min_wavefront_length=0), 850),
    ("gcd3", dict(mismatch=6, gap_opening=9, gap_extension=3), 700),
    ("gcd3-complete", dict(mismatch=6, gap_opening=9, gap_extension=3, min_wavefront_length=0), 700),
    ("x7-o1-e5", dict(mismatch=7, gap_opening=1, gap_extension=5), 100),
    ("x7-o1-e5-complete", dict(mismatch=7, gap_opening=1, gap_extension=5, min_wavefront_length=0), 100),
    ("x1-o0-e1", dict(mismatch=1, gap_opening=0, gap_extension=1), 100),
    ("x1-o0-e1-complete", dict(mismatch=1, gap_opening=0, gap_extension=1, min_wavefront_length=0), 100),
]
C_NAMES = [c[0] for c in C_SETS]


def group_c(name):
    """one N run from site 300, alone and followed by a deletion of four sites and an insertion of three characters"""
    _, opts, n = C_SETS[C_NAMES.index(name)]
    ref = F.random_acgt(C_LEN, 20261205)
    q = n_run(ref, 300, n)
    q2 = q[:1300] + q[1304:1400] + b"GAT" + q[1400:]
    return [Pool("C-" + name, ref, dict(opts), (q, q2))]


# ---------------------------------------------------------------------------------------------------------------- D: extension
D_LEN = 5000
D_RUNS = (0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 519, 520, 521, 1023, 1024, 1025, 1031, 1032, 1033, 2047, 2048, 2049, 2055, 2056, 2057)
D_ENDS = ("mismatch", "both", "query", "reference")
D_DIAGONALS = (0, 3, -5)
D_TAIL = 30                 # sites of the reference after a run that ends inside it
# a query of one character against 5 000 sites is a gap of 4 999: 4.9 M cells, 13 chunks of history.  The pool holds a thousand of them, so
# this group's aligner gets a workspace in which 32 such queries in flight find their chunks (pool_fits; the CPU test checks it).
D_OPTS = dict(workspace_bytes=1 << 30, max_blocks=32)


def d_query(ref, run, end, diag):
    """(query, the query to put next in the pool or None).  The run of `run` matches starts right after a substituted site; a short insertion
    or deletion 40 sites before it moves it to another diagonal."""
    L = len(ref)
    p = L - run if end in ("both", "reference") else L - run - D_TAIL        # the run is ref[p:p + run]
    cut = p - 40
    if diag > 0:
        head = ref[:cut] + other(ref[cut:cut + 1]) * diag                           # an insertion: the run lies on diagonal +diag
    else:
        head = ref[:cut + diag]                                                     # a deletion of -diag sites (or nothing)
    q = head + ref[cut:p - 1] + other(ref[p - 1:p]) + ref[p:p + run]
    nxt = None
    if end == "mismatch":
        q += other(ref[p + run:p + run + 1]) + ref[p + run + 1:]
    elif end == "reference":
        q += b"GATTACAGATTA"                                                        # characters beyond the reference's end
    elif end == "query":                                                            # the next query goes on where the reference does
        nxt = ref[p + run:] + ref[D_TAIL:]
    return q, nxt


@functools.lru_cache(maxsize=None)
def group_d():
    """the pool: before every query 0 .. 7 queries of one character, as many as put its first character at an address that is i modulo 8
    for the i-th query built (the pool's buffer is aligned: uvaia_align_load_block copies it to the start of an allocation); after every
    query that ends inside the reference one that starts with the sites that follow.  Returns (pools, (position, run, end, diagonal) of
    the built queries)."""
    ref = F.random_acgt(D_LEN, 20261206)
    seqs, built, i, at = [], [], 0, 0
    for run in D_RUNS:
        for end in D_ENDS:
            for diag in D_DIAGONALS:
                pads = [b"ACGT"[j % 4:j % 4 + 1] for j in range((i - at) % 8)]
                seqs += pads
                at += len(pads)
                q, nxt = d_query(ref, run, end, diag)
                built.append((len(seqs), run, end, diag))
                at += len(q) + (len(nxt) if nxt is not None else 0)
                seqs.append(q)
                if nxt is not None:
                    seqs.append(nxt)
                i += 1
    return [Pool("D", ref, dict(D_OPTS), tuple(seqs))], built


# ---------------------------------------------------------------------------------------------------------------- E: backtrace
E_LEN = 700
E_RUNS = (1, 2, 62, 63, 64, 65, 125, 126, 127, 128, 189, 190)
E_GAPS = (1, 2, 63, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def group_e_cases():
    """(reference, list of (query, closed form of its score or None))"""
    ref = F.random_acgt(E_LEN, 20261207)
    junk = F.random_acgt(300, 20261208)
    d = DEFAULTS
    out, seen = [], set()
    for n in E_RUNS:
        for a in (0, 1, 300, E_LEN - 1 - n, E_LEN - n):
            q = n_run(ref, a, n)
            if q not in seen:
                seen.add(q)
                out.append((q, d["mismatch"] * n))
    out.append((n_run(n_run(ref, 100, 63), 164, 64), d["mismatch"] * 127))                # two runs, one matching site between them
    out.append((ref[:200] + b"N" * 64 + ref[274:], None))                                 # a run abutting a deletion
    out.append((ref[:200] + b"N" * 64 + other(ref[264:269]) + ref[264:], None))           # a run abutting an insertion
    for n in E_GAPS:
        cost = d["gap_opening"] + d["gap_extension"] * n
        out += [(ref[n:], cost), (ref[:350] + ref[350 + n:], cost), (ref[:E_LEN - n], cost)]
        out += [(junk[:n] + ref, cost), (ref[:350] + junk[:n] + ref[350:], cost), (ref + junk[:n], cost)]
    out += [(b"N" * 699, None), (b"N" * 700, d["mismatch"] * 700), (b"N" * 701, None)]
    out.append((b"", d["gap_opening"] + d["gap_extension"] * E_LEN))
    out += [(c, None) for c in (b"A", b"C", b"G", b"T", b"N")]
    out.append((n_run(ref, 50, 600), d["mismatch"] * 600))                                # scores 0 .. 2 400 along one diagonal
    return ref, out


def group_e(complete=False):
    ref, cases = group_e_cases()
    opts = dict(min_wavefront_length=0) if complete else {}
    one = b"A"
    return [Pool("E", ref, opts, tuple(q for q, _ in cases)), Pool("E-one-site", one, opts, (b"A", b"C", b"N", b"AC", b"CA", b"AA", b"CG"))]
