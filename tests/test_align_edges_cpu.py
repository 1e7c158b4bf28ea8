"""The inputs of tests/align_edges.py, on the CPU: every one reaches the edge of wfa_align_kernel it is built for (shown through the path
model, align_edges.step_paths, over the oracle's per-score limits), none would be refused by the kernel, the oracle agrees with the Gotoh
recurrence and with closed forms where those apply, and orc_wfa_limits agrees with the oracle's own counters.  The device runs the same
inputs in tests/test_align_edges_gpu.py."""
import functools

import pytest

import align_edges as AE
import oracle_lib as O


@functools.lru_cache(maxsize=None)
def _paths(ref, seq, opts_key):
    return AE.paths(ref, seq, dict(opts_key))


def pool_paths(pool):
    return [_paths(pool.ref, q, tuple(sorted(pool.opts.items()))) for q in pool.seqs]


def all_pools():
    pools = list(AE.group_a())
    for s in AE.B_SETTINGS:
        pools += AE.group_b(s)
    pools += AE.group_b_outside()
    for name in AE.C_NAMES:
        pools += AE.group_c(name)
    pools += AE.group_d()[0] + AE.group_e() + AE.group_e(complete=True)
    return pools


def check_pool(pool):
    """consistency of orc_wfa_limits with the oracle's counters, and the kernel's legal range"""
    pp = pool_paths(pool)
    for q, p in zip(pool.seqs, pp):
        widths = [t[2] - t[1] + 1 for t in p.shape]
        assert p.score >= 0 and p.shape[-1][0] == p.score
        assert sum(widths) == p.cells and max(widths) == p.width, (pool.name, len(q))
        assert all(t[1] <= t[3] <= t[4] <= t[2] for t in p.shape)
        assert len(p.steps) == len(p.shape) and p.steps[-1].refused is None, (pool.name, len(q), p.steps[-1].refused)
        assert [s.w for s in p.steps] == widths
        assert p.steps[-1].pages <= AE.MAX_HDR_PAGES and p.steps[-1].chunks <= AE.MAX_OWN
    assert AE.pool_fits([p.steps[-1].chunks for p in pp], len(pool.ref), pool.opts), pool.name
    return pp


# ---------------------------------------------------------------------------------------------------------------------------- A
def test_a_offsets_leave_16_bits_in_mid_flight_at_the_start_and_before_it():
    pool, = AE.group_a()
    pp = check_pool(pool)
    fits = [[s.fits for s in p.steps] for p in pp]
    assert [len(q) for q in pool.seqs] == [65400, 65502, 65503, 65535, 65536, 65593, 65700]
    # 65 400 characters: `tlen + step + 32 < 65535` holds for steps 0 .. 102 and the query goes on for hundreds of steps, in both bodies
    assert fits[0][:103] == [True] * 103 and not any(fits[0][103:]) and len(fits[0]) > 400
    assert any(s.lds_only for s in pp[0].steps) and not pp[0].steps[103].resident and pp[0].steps[103].id_to_memory
    # steps after the loss read wavefronts that are still in LDS next to ones that never were
    assert any(not s.resident and not (s.mem_s and s.mem_g and s.mem_e) for s in pp[0].steps[103:108])
    assert fits[1][0] and not any(fits[1][1:])                              # 65 502: step 0 only
    assert all(not any(f) for f in fits[2:])                                # 65 503 and longer: never
    assert sum(len(q) > 65535 for q in pool.seqs) == 3                      # offsets that no 16 bits hold
    assert AE.chunk_log2(len(pool.ref), 2) == 21                            # chunks of 8 MB


# ---------------------------------------------------------------------------------------------------------------------------- B
def test_b_complete_wavefronts_cross_the_lds_width():
    pool, = AE.group_b(AE.B_SETTINGS[0])
    p, = check_pool(pool)
    i = [s.w for s in p.steps].index(2559)
    assert p.steps[i].resident and p.steps[i].lds_only and p.steps[i + 1].w == 2561 and not p.steps[i + 1].resident
    assert not p.steps[i + 1].mem_s and p.steps[i + 6].mem_s and p.steps[i + 6].mem_g and p.steps[i + 6].mem_e     # sources leave LDS one by one
    assert p.steps[-1].wraps >= 2 and p.steps[-1].chunks >= 2 and p.width > 2 * AE.WL


@pytest.mark.parametrize("min_len", AE.B_MIN_LEN)
def test_b_first_reduction_acts_on_the_intended_width(min_len):
    seen = set()
    for max_dist in AE.B_MAX_DIST:
        pool, = AE.group_b(dict(min_wavefront_length=min_len, max_distance_threshold=max_dist))
        p, = check_pool(pool)
        first = next(i for i, t in enumerate(p.shape) if t[2] - t[1] + 1 >= min_len)
        assert all(t[1] == t[3] and t[2] == t[4] for t in p.shape[:first])                  # untouched before
        t = p.shape[first]
        assert t[2] - t[1] + 1 == max(min_len | 1, 3 if min_len > 1 else 1)                 # widths grow 1, 3, 5, ...: the first one >= min_len
        if max_dist <= 1 and min_len > 1:
            assert t[4] - t[3] < t[2] - t[1]                                                # and it is trimmed there
        seen.add((p.score, p.cells, p.width))
    assert len(seen) >= 2                                                                    # the threshold matters


def test_b_reduction_flips_residency_back_and_forth():
    pool, = AE.group_b(dict(min_wavefront_length=2560, max_distance_threshold=512))
    p, = check_pool(pool)
    res = [s.resident for s in p.steps]
    flips = sum(a != b for a, b in zip(res, res[1:]))
    assert flips >= 4 and p.width > AE.WL
    back = [s for a, s in zip(p.steps, p.steps[1:]) if not a.resident and s.resident]
    assert back and all(s.mem_s or s.mem_g or s.mem_e for s in back)                         # a resident step reads a source from memory
    assert any(s.resident and not s.lds_only and not s.id_to_memory for s in p.steps)
    triples = set()
    for s in AE.B_SETTINGS[1:]:
        q, = pool_paths(AE.group_b(s)[0])
        triples.add((q.score, q.cells, q.width))
    assert len(triples) >= 40                                                                # the sweep is no repetition of one run


def test_b_end_diagonal_outside_the_first_reduced_wavefronts():
    for pool in AE.group_b_outside():
        p, = check_pool(pool)
        k_end = len(pool.seqs[0]) - len(pool.ref)
        assert abs(k_end) == 2000 and p.score == 2 * 6 + 2 * 2000
        first = next(t for t in p.shape if t[2] - t[1] + 1 >= 128)
        assert not first[1] <= k_end <= first[2]                                             # not even allocated yet


# ---------------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", AE.C_NAMES)
def test_c_penalty_sets(name):
    pool, = AE.group_c(name)
    pp = check_pool(pool)
    x, o, e = AE.penalties_of(pool.opts)
    g = AE.gcd3(x, o + e, e)
    st = pp[0].steps
    if name == "deep-ring-wrap":
        assert pp[0].score == 800 and pp[0].width == 801 and all(s.id_to_memory and not s.lds_only for s in st)
        assert st[-1].wraps == 1            # one wrap only: sum of 2 * w16 over the 794 steps is 656 000 words, a chunk is 524 288
    if name == "deep-ring-wrap-600":
        assert all(s.id_to_memory and s.resident and not s.lds_only for s in st) and st[-1].wraps >= 2 and pp[1].steps[-1].wraps >= 2
        assert any(s.mem_e and s.resident for s in st) and any(s.mem_g and s.resident for s in st)
    if name.startswith("ring-edge"):
        assert x == AE.RING - 1 and o + e == AE.RING - 1
        for what in ("mem_s", "mem_g", "mem_e"):
            assert any(getattr(s, what) and s.resident for s in st), what
        assert any(not s.mem_s and s.score >= x for s in st)
    if name.startswith("gcd"):
        assert g in (3, 5) and pp[0].score > 4096
        opened = sorted({s.page_at for s in st})
        assert len(opened) == 3 and all(a % AE.HDR_PAGE_SCORES != 0 and a % g == 0 for a in opened[1:])
        assert any(s.lds_only for s in st) and any(not s.lds_only for s in st)              # both bodies within one query
    if name == "gcd3-complete":
        assert pp[0].width > AE.WL and any(not s.resident for s in st)
    if name.startswith("x7-o1-e5"):
        assert e // g >= AE.RID and any(s.mem_s and s.mem_g and s.mem_e and s.resident for s in st)


# ------------------------------------------------------------------------------------------------------------------------ D, E
def test_d_runs_end_where_they_should_on_every_address_residue():
    (pool,), built = AE.group_d()
    pp = check_pool(pool)
    off = [0]
    for q in pool.seqs:
        off.append(off[-1] + len(q))
    assert [off[i] % 8 for i, _, _, _ in built] == [j % 8 for j in range(len(built))]
    assert len(built) == len(AE.D_RUNS) * 4 * 3
    for i, run, end, diag in built:
        q, cigar = pool.seqs[i], pp[i].cigar
        assert O.cigar_score(cigar, pool.ref, q) == pp[i].score
        if end == "mismatch":
            assert b"X" + b"M" * run + b"X" in cigar
        elif end == "both":
            assert cigar.endswith(b"X" + b"M" * run)
        elif end == "query":                         # the query ends with the run; what follows it in the pool goes on matching the reference
            a = len(pool.ref) - AE.D_TAIL
            assert q.endswith(pool.ref[a - run:a]) and pool.seqs[i + 1].startswith(pool.ref[a:]) and len(pool.seqs[i + 1]) > 1
        else:
            assert len(q) > len(pool.ref) - diag - 1 and q[:-12].endswith(pool.ref[len(pool.ref) - run:])
        assert (b"I" * 3 in cigar) if diag == 3 else (b"D" * 5 in cigar) if diag == -5 else True


def test_e_closed_forms():
    ref, cases = AE.group_e_cases()
    for complete in (False, True):
        pools = AE.group_e(complete)
        pp = check_pool(pools[0])
        check_pool(pools[1])
        for (q, want), p in zip(cases, pp):
            if want is not None:
                assert p.score == want, (len(q), p.score, want)
    assert sum(want is not None for _, want in cases) > 90
    p = pp[[q for q, _ in cases].index(b"")]
    assert p.cigar == b"D" * len(ref)
    run600 = _paths(ref, cases[-1][0], ())
    assert run600.cigar.count(b"X") == 600 and run600.score > AE.HDR_PAGE_SCORES and run600.steps[-1].pages == 2


# ---------------------------------------------------------------------------------------------------------------- the whole module
def test_both_step_bodies_within_one_query_and_pages_off_the_page_size():
    mixed = pages_off = 0
    for pool in all_pools():
        for p in pool_paths(pool):
            kinds = {s.lds_only for s in p.steps}
            mixed += len(kinds) == 2 and sum(a.lds_only != b.lds_only for a, b in zip(p.steps, p.steps[1:])) >= 3    # alternating, not one switch
            pages_off += any(s.page_at % AE.HDR_PAGE_SCORES for s in p.steps)
    assert mixed > 20 and pages_off >= 4


def test_oracle_against_gotoh_and_its_own_cigar():
    """every pair small enough for the full table: the CIGAR spells the pair at the reported score under the penalties used; with complete
    wavefronts the score is the optimum of the Gotoh recurrence"""
    n_gotoh = n_cigar = 0
    for pool in all_pools():
        pen = (0,) + AE.penalties_of(pool.opts)
        for q in set(pool.seqs):
            if len(pool.ref) * len(q) > AE.GOTOH_CELLS:
                continue
            score, _, _, _, cigar = AE.expected(pool.ref, q, pool.opts)
            assert O.cigar_score(cigar, pool.ref, q, pen) == score
            n_cigar += 1
            if AE.is_complete(pool.opts):
                assert O.gotoh_score(pool.ref, q, pen) == score, (pool.name, len(q))
                n_gotoh += 1
    assert n_gotoh > 100 and n_cigar > 200


def test_limits_of_a_score_without_wavefronts():
    score, cigar, shape = O.wfa_shape(b"ACGTACGTAC", b"ACGTTCGAC")
    assert score == 12 and [t[0] for t in shape] == [0, 4, 8, 10, 12]
    assert shape[0] == (0, 0, 0, 0, 0, False, False) and shape[1][5:] == (False, False) and shape[2][5:] == (True, True)
    assert (score, cigar) == O.wfa_align(b"ACGTACGTAC", b"ACGTTCGAC")[:2]
