"""The compact form of a packed database written from device memory, on a GPU box: uvaia_gpu_db_encode_compact + uvaia_gpu_db_encoded_records
(encode_count_kernel, encode_prefix_kernel, encode_emit_kernel) against the records the host writer (compact_lib.write_compact) gives the
same references, and the command lines that take the device route: `uvaialign --packed --compact`, `uvaiaclust --packed-out --compact`,
`uvaiapack --compact` and `uvaiapack --merge --compact`.  The reference of every comparison is the host path: packed_lib.pack_tiles for
dense tiles, compact_lib.write_compact for records, `uvaiapack` for whole files."""
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import compact_lib as CL
import fixtures as F
import oracle_lib as O
import packed_lib as P
import rows_lib as R
from uvaia_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _queries(nchar, n=3):
    root = bytes(b"ACGT"[s & 3] for s in range(nchar))
    return [root] * n, ["q%d" % i for i in range(n)]


def _engine(nchar, **kw):
    qs, qn = _queries(nchar)
    return capi.Engine.from_query(O.Query(qs, qn, **kw), nbest=2, max_pool=64)


# ---------------------------------------------------------------------------------------------------------------- rows
def _hand_made(root):
    """rows that differ from `root` (the base, as long as most rows equal it) in chosen words; with fewer words than a shape needs the
    row keeps what fits"""
    nchar, out = len(root), []
    n_real = (nchar + 31) // 32
    other = lambda ch: ord("A") if ch != ord("A") else ord("C")

    def word_n(s, w):
        if w < n_real:
            s[32 * w:32 * w + 32] = b"N" * len(s[32 * w:32 * w + 32])

    def word_all(s, w, ch):
        if w < n_real:
            s[32 * w:32 * w + 32] = ch * len(s[32 * w:32 * w + 32])

    def word_lit(s, w, code=b"R"):
        if w < n_real:
            s[min(32 * w + 5, nchar - 1)] = code[0]

    out.append(bytes(root))                                                        # equal to the base: no head
    s = bytearray(root)
    for w in range(n_real):
        s[32 * w] = other(s[32 * w])                                               # differs in every word: one literal head of all words
    out.append(bytes(s))
    s = bytearray(root); word_n(s, 0); word_lit(s, 1); word_lit(s, 3); word_n(s, 4)      # fill -> literal, literal -> fill in adjacent words
    out.append(bytes(s))
    s = bytearray(root); word_n(s, 0); word_all(s, 1, b"A"); word_all(s, 2, b"B"); word_all(s, 3, b"N")    # fill (code 0) -> fill (code 1) -> fill (code 14) -> fill (0)
    out.append(bytes(s))
    s = bytearray(root); word_lit(s, 0); word_lit(s, 2); word_n(s, 4); word_n(s, 6)      # one equal word between two runs
    out.append(bytes(s))
    s = bytearray(root); word_n(s, n_real - 1); word_n(s, n_real - 2)              # a run ending in the last real word
    out.append(bytes(s))
    s = bytearray(root); word_lit(s, n_real - 1, b"Y")
    out.append(bytes(s))
    out.append(b"A" * nchar)                                                        # a partial last word of all A is a literal, not a fill
    out.append(b"N" * nchar)
    return out


def _rows(n, nchar, seed):
    """n references of one lineage, the hand-made rows spread among them where n allows; the first row is the root"""
    rng = np.random.default_rng(seed)
    root = rng.choice(ACGT, size=nchar).tobytes()
    seqs = [root] + [s.upper() for s in CL.near_identical_references(max(n - 1, 0), nchar, seed + 1)]
    # near_identical_references draws its own root: put every row on this one so that the majority base is `root`
    seqs = [root if i % 3 else s for i, s in enumerate(seqs)][:n]
    hand = _hand_made(root)
    step = max(1, n // (len(hand) + 1))
    for k, h in enumerate(hand):
        i = 1 + k * step
        if i < n:
            seqs[i] = h
    return seqs


def _host_file(tmp, seqs, tag):
    nchar = len(seqs[0])
    planes, non_n = P.pack_tiles(seqs, nchar)
    path = tmp / ("%s.uvdb" % tag)
    CL.write_compact(path, ["r%d" % i for i in range(len(seqs))], seqs, planes, non_n)
    return planes, non_n, CL.CompactFile(path)


def _lane_records(head_idx, heads, lit_idx, lits, g):
    lits = np.asarray(lits, dtype=np.uint32).reshape(-1, 4)
    return ([int(h) for h in heads[int(head_idx[g]):int(head_idx[g + 1])]], lits[int(lit_idx[g]):int(lit_idx[g + 1])].tolist())


def _encode(eng, base, first_tile=0, n_tiles=None):
    hi, li, nn = eng.db_encode_compact(base, first_tile, n_tiles)
    heads, lits = eng.db_encoded_records()
    assert hi[0] == 0 and li[0] == 0 and len(heads) == int(hi[-1]) and lits.shape == (int(li[-1]), 4)
    return hi, li, nn, heads, lits


def _assert_is_the_host_file(got, cf, t0, nt, note):
    """records of tiles t0 .. t0 + nt - 1 against the sections of the host-written file: both indices, every head, every literal, non_n"""
    hi, li, nn, heads, lits = got
    a, b = t0 * 64, (t0 + nt) * 64
    assert np.array_equal(hi, cf.head_idx[a:b + 1] - cf.head_idx[a]), (note, "head_idx")
    assert np.array_equal(li, cf.lit_idx[a:b + 1] - cf.lit_idx[a]), (note, "lit_idx")
    assert np.array_equal(heads, cf.heads[int(cf.head_idx[a]):int(cf.head_idx[b])]), (note, "heads")
    assert np.array_equal(lits.reshape(-1), cf.lits[int(cf.lit_idx[a]) * 4:int(cf.lit_idx[b]) * 4]), (note, "lits")
    assert np.array_equal(nn, cf.non_n[a:b]), (note, "non_n")


def _assert_against_a_forced_base(tmp, eng, seqs, base_row, tag):
    """The host writer's base is the majority of its first rows: a file of len(seqs) + 65 copies of base_row, then seqs, then 64 all-N rows
    (the planes of a zero lane) has base_row's planes as its base and holds, from lane len(seqs) + 65 on, the records of the engine's lanes."""
    n, nchar = len(seqs), len(seqs[0])
    shift = n + 65
    _, _, cf = _host_file(tmp, [base_row] * shift + seqs + [b"N" * nchar] * 64, tag)
    assert np.array_equal(cf.base, P.pack_tiles([base_row], nchar)[0].reshape(-1).view(np.uint32).reshape(-1, 4, 64, 4)[:, :, 0, :].reshape(-1))
    hi, li, nn, heads, lits = _encode(eng, cf.base)
    for g in range(len(hi) - 1):
        want = _lane_records(cf.head_idx, cf.heads, cf.lit_idx, cf.lits, shift + g)
        assert _lane_records(hi, heads, li, lits, g) == want, (tag, "lane", g)
        assert nn[g] == cf.non_n[shift + g], (tag, "non_n", g)
    return cf.base, hi, li, nn, heads, lits


# ---------------------------------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize("nchar", [29, 32, 33, 127, 128, 129, 1000])
def test_records_are_the_host_writers(tmp_path, nchar):
    rng = np.random.default_rng(nchar)
    with _engine(nchar) as eng:
        eng.db_reserve(192)
        eng.db_stage_reserve(3)
        for n in (1, 63, 64, 65, 130):
            seqs = _rows(n, nchar, 1000 * nchar + n)
            planes, non_n, cf = _host_file(tmp_path, seqs, "own%d" % n)
            nt = planes.shape[0]
            eng.db_clear()
            eng.db_append(seqs)
            dense = eng.db_export()
            assert np.array_equal(dense[0], planes) and np.array_equal(dense[1], non_n)
            # the file's own base: the sections as they stand, the zero lanes behind the last reference included
            got = _encode(eng, cf.base)
            _assert_is_the_host_file(got, cf, 0, nt, (nchar, n))
            if n >= 64:
                hand = [i for i in range(n) if cf.heads_of(i)]
                assert len(hand) >= 6 and not cf.heads_of(0)                       # the hand-made rows left heads, the root none
            # any other base: all zeros, a random row, one of the rows
            random_row = np.frombuffer(P.CODE[1:15], dtype=np.uint8)[rng.integers(0, 14, size=nchar)].tobytes()
            for tag, base_row in (("zero", b"N" * nchar), ("random", random_row), ("row", seqs[n // 2])):
                forced = _assert_against_a_forced_base(tmp_path, eng, seqs, base_row, "%s%d" % (tag, n))
                # round trip: the records expand to the tiles they were made of
                base, hi, li, nn, heads, lits = forced
                eng.db_stage_compact_at(0, 0, base, hi, heads if len(heads) else np.zeros(1, np.uint32), li,
                                        lits.reshape(-1) if len(lits) else np.zeros(4, np.uint32), nn, nt)
                eng.db_clear()
                eng.db_append_staged(0, None, n)
                back = eng.db_export()
                for x, y, what in zip(back, (planes, non_n, CL.side_rows_canonical(planes, nchar)), ("planes", "non_n", "side rows")):
                    assert np.array_equal(x, y), (nchar, n, tag, what)
                eng.db_clear()
                eng.db_append(seqs)
        ms = eng.encode_ms()
        assert ms[0] > 0 and ms[1] > 0


def test_hand_made_rows_encode_as_designed(tmp_path):
    """what the host writer makes of the hand-made rows (so that the comparison above covers the shapes it claims to), at 1 000 sites"""
    nchar = 1000
    seqs = _rows(130, nchar, 5)
    _, _, cf = _host_file(tmp_path, seqs, "designed")
    step, n_real = 130 // 10, 32
    at = lambda k: cf.heads_of(1 + k * step)
    assert at(0) == [] and at(1) == [(0, n_real, 1, 0)]
    assert at(2) == [(0, 1, 0, 0), (1, 1, 1, 0), (3, 1, 1, 0), (4, 1, 0, 0)]
    assert at(3) == [(0, 1, 0, 0), (1, 1, 0, 1), (2, 1, 0, 14), (3, 1, 0, 0)]
    assert at(4) == [(0, 1, 1, 0), (2, 1, 1, 0), (4, 1, 0, 0), (6, 1, 0, 0)]
    assert at(5) == [(n_real - 2, 2, 0, 0)] and at(6) == [(n_real - 1, 1, 1, 0)]
    assert at(7)[-1][:3] == (n_real - 1, 1, 1) and all(h[2] == 1 or h[3] == 1 for h in at(7))     # all A: the partial last word is a literal
    assert at(8) == [(0, n_real, 0, 0)]


def test_heads_are_cut_at_2047_words(tmp_path):
    nchar = 70000
    n_real = (nchar + 31) // 32                                                    # 2 188 words
    root = np.random.default_rng(9).choice(ACGT, size=nchar).tobytes()
    every = bytearray(root)
    for w in range(n_real):
        every[32 * w + 3] = ord("R")
    seqs = [root, b"N" * nchar, bytes(every), root, root]
    planes, non_n, cf = _host_file(tmp_path, seqs, "cut")
    assert cf.heads_of(1) == [(0, 2047, 0, 0), (2047, 141, 0, 0)] and cf.heads_of(2) == [(0, 2047, 1, 0), (2047, 141, 1, 0)]
    with _engine(nchar) as eng:
        eng.db_reserve(64)
        eng.db_append(seqs)
        assert np.array_equal(eng.db_export()[0], planes)
        _assert_is_the_host_file(_encode(eng, cf.base), cf, 0, 1, "cut")


def test_prefix_pass_across_blocks(tmp_path):
    nchar, n = 33, 65 * 64 - 7                                                     # 4 160 lanes: more than four rounds of the prefix block
    seqs = _rows(n, nchar, 77)
    planes, non_n, cf = _host_file(tmp_path, seqs, "prefix")
    assert int(cf.head_idx[-1]) > 1024
    with _engine(nchar) as eng:
        eng.db_reserve(n)
        eng.db_append_packed(planes, non_n, CL.side_rows_canonical(planes, nchar), n)
        _assert_is_the_host_file(_encode(eng, cf.base), cf, 0, 65, "prefix")
        _assert_is_the_host_file(_encode(eng, cf.base, 17, 40), cf, 17, 40, "prefix, tiles 17..56")


def test_tile_range_and_stale_lanes(tmp_path):
    nchar = 129
    seqs = _rows(200, nchar, 31)
    planes, non_n, cf = _host_file(tmp_path, seqs[:130], "three")
    with _engine(nchar) as eng:
        eng.db_reserve(256)
        eng.db_append(seqs[:130])
        _assert_is_the_host_file(_encode(eng, cf.base, 1, 2), cf, 1, 2, "tiles 1..2 of 3")
        # 130 appended, two tiles dropped, 70 more appended: references 128, 129, then 130 .. 199; the lanes behind them are zero rows
        eng.db_drop_tiles(2)
        eng.db_append(seqs[130:200])
        assert eng.db_size() == 72
        now = seqs[128:200]
        planes2, non_n2, cf2 = _host_file(tmp_path, now, "after_drop")
        got = _encode(eng, cf2.base)
        _assert_is_the_host_file(got, cf2, 0, 2, "after a drop")
        zero = _lane_records(cf2.head_idx, cf2.heads, cf2.lit_idx, cf2.lits, 127)
        assert all(_lane_records(got[0], got[3], got[1], got[4], g) == zero for g in range(72, 128)) and not got[2][72:].any()
        # the same tiles against the base of the other file: still the host's records
        _assert_against_a_forced_base(tmp_path, eng, now, seqs[5], "after_drop_other_base")


def test_refusals_leave_the_context_usable(tmp_path):
    nchar = 129
    seqs = _rows(70, nchar, 41)
    planes, non_n, cf = _host_file(tmp_path, seqs, "refusals")
    with _engine(nchar, acgt=True) as eng:                                         # an --acgt context keeps three planes: nothing to encode from
        with pytest.raises(capi.GpuError):
            eng.db_encode_compact(cf.base, 0, 0)
        with pytest.raises(capi.GpuError):
            eng.db_encoded_records()
        assert eng.db_size() == 0
    with _engine(nchar) as eng:
        eng.db_reserve(192)
        with pytest.raises(capi.GpuError):                                         # records without a plan
            eng.db_encoded_records()
        eng.db_append(seqs)
        with pytest.raises(capi.GpuError):                                         # tiles outside the database
            eng.db_encode_compact(cf.base, 1, 2)
        with pytest.raises(capi.GpuError):
            eng.db_encode_compact(cf.base, 3, 1)
        with pytest.raises(capi.GpuError):                                         # the refused plan is no plan
            eng.db_encoded_records()
        hi, li, nn = eng.db_encode_compact(cf.base)
        eng.db_append(seqs[:3])                                                    # the database changed: the plan is void
        with pytest.raises(capi.GpuError):
            eng.db_encoded_records()
        eng.db_encode_compact(cf.base)
        eng.db_drop_tiles(1)
        with pytest.raises(capi.GpuError):
            eng.db_encoded_records()
        eng.db_encode_compact(cf.base, 0, 1)
        eng.db_clear()
        with pytest.raises(capi.GpuError):
            eng.db_encoded_records()
        # and the context works afterwards
        eng.db_append(seqs)
        _assert_is_the_host_file(_encode(eng, cf.base), cf, 0, 2, "after the refusals")
        assert np.array_equal(eng.db_export()[0], planes)


# ---------------------------------------------------------------------------------------------------------------- command lines
def _write_fasta(path, names, seqs, opener=open):
    with opener(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd, env=None):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900, env=env)
    assert r.returncode == 0, (cmd, r.stderr[-3000:])
    return r.stderr.decode(errors="replace")


def _routes(err):
    """(tiles encoded on the device, tiles encoded on the host) from a command's closing lines"""
    m = re.search(r"[Cc]ompact tiles: (\d+) encoded on the device.*?(\d+) on the host", err)
    assert m, err[-2000:]
    return int(m.group(1)), int(m.group(2))


def _xz(path):
    return lzma.open(str(path), "rb").read()


def _lineage(n, nchar, seed, private):
    """aligned rows of one lineage: a root with `private` substitutions of its own per row, a short N run at either end now and then, an
    IUPAC code here and there, a short gap in some: every row passes -A 0.5"""
    rng = np.random.default_rng(seed)
    root = rng.choice(ACGT, size=nchar)
    out = []
    for i in range(n):
        s = root.copy()
        pos = rng.choice(nchar, size=private, replace=False)
        s[pos] = ACGT[(np.searchsorted(ACGT, s[pos]) + rng.integers(1, 4, size=private)) % 4]
        if i % 4 == 1:
            s[:int(rng.integers(1, 40))] = ord("N")
        if i % 6 == 2:
            s[nchar - int(rng.integers(1, 40)):] = ord("N")
        if i % 9 == 4:
            s[int(rng.integers(0, nchar))] = rng.choice(np.frombuffer(b"RYKMSW", dtype=np.uint8))
        if i % 13 == 5:
            a = int(rng.integers(40, nchar - 60))
            s[a:a + int(rng.integers(1, 12))] = ord("-")
        out.append(s.tobytes())
    return out


N_SEQ, AMBIG_R = 4400, "0.3"


@pytest.fixture(scope="module")
def aligned(tmp_path_factory):
    """one reference of 350 sites and 4 400 unaligned sequences in two files; the text and the two-step compact file of `uvaialign -o` +
    `uvaiapack --compact`, and the dense file"""
    d = tmp_path_factory.mktemp("encode_align")
    ref = F.random_acgt(350, 51)
    seqs = F.unaligned_queries(ref, N_SEQ, 52, p_snp=0.004, p_indel=0.001, max_indel=6, n_runs=(20, 20, 40))
    for i in range(7, N_SEQ, 40):                                                   # some fail -A 0.3 and pass the aligner's -a 0.5
        s = bytearray(seqs[i]); k = (4 * len(s)) // 10; s[20:20 + k] = b"N" * k; seqs[i] = bytes(s)
    names = ["seq %d|2021" % i for i in range(N_SEQ)]
    _write_fasta(d / "ref.fa", ["the reference"], [ref])
    _write_fasta(d / "raw1.fa", names[:3000], seqs[:3000])
    _write_fasta(d / "raw2.fa.xz", names[3000:], seqs[3000:], opener=lzma.open)
    _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw1.fa"), str(d / "raw2.fa.xz"), "-o", str(d / "t"), "-p", "512"])
    _run([UVAIAPACK, "-A", AMBIG_R, "--compact", "-o", str(d / "b.uvdb"), str(d / "t.aln.xz")])
    _run([UVAIAPACK, "-A", AMBIG_R, "-o", str(d / "dense.uvdb"), str(d / "t.aln.xz")])
    return d, ref


def _align_compact(d, tag, extra):
    path = d / ("a_%s.uvdb" % tag)
    err = _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw1.fa"), str(d / "raw2.fa.xz"), "--packed", str(path), "--compact", "-A", AMBIG_R] + extra)
    return path, err


def test_the_aligned_input_keeps_enough_for_the_device_route(aligned):
    d, ref = aligned
    names, rows = F.read_fasta_bytes(_xz(d / "t.aln.xz"))
    kept = [r for r in rows if R.count_non_n(r) >= int(len(ref) * (1 - float(AMBIG_R)))]
    assert len(kept) > 4096 + 64 and len(rows) - len(kept) >= 50
    assert CL.file_version(str(d / "b.uvdb")) == 2 and CL.CompactFile(d / "b.uvdb").n_ref == len(kept)
    assert sum(1 for r in kept if b"-" in r) > 100


@pytest.mark.parametrize("pool", [37, 64, 100000])
def test_uvaialign_compact_is_the_two_step_file_whatever_the_pool(aligned, pool):
    d, _ = aligned
    path, err = _align_compact(d, "p%d" % pool, ["-p", str(pool)])
    assert path.read_bytes() == (d / "b.uvdb").read_bytes()
    dev, host = _routes(err)
    assert dev > 0 and host >= 64 and dev + host == CL.CompactFile(path).n_tiles


def test_uvaialign_compact_with_text_next_to_it(aligned):
    d, _ = aligned
    path, err = _align_compact(d, "with_text", ["-p", "300", "-o", str(d / "t2")])
    assert path.read_bytes() == (d / "b.uvdb").read_bytes() and _routes(err)[0] > 0
    assert _xz(d / "t2.aln.xz") == _xz(d / "t.aln.xz")


def test_uvaialign_compact_below_the_sample_takes_the_host_route(tmp_path):
    """the 330-sequence shape of test_align_packed_gpu.py: the base is fixed at close, every tile is encoded on the host, the file is equal"""
    d = tmp_path
    ref = F.random_acgt(2003, 31)
    seqs = F.unaligned_queries(ref, 330, 32, p_indel=0.0015, n_runs=(30, 30, 100))
    _write_fasta(d / "ref.fa", ["the reference"], [ref])
    _write_fasta(d / "raw.fa", ["s %d" % i for i in range(330)], seqs)
    _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw.fa"), "-o", str(d / "t"), "-p", "64"])
    _run([UVAIAPACK, "-A", "0.2", "--compact", "-o", str(d / "b.uvdb"), str(d / "t.aln.xz")])
    err = _run([UVAIALIGN, "-r", str(d / "ref.fa"), str(d / "raw.fa"), "--packed", str(d / "a.uvdb"), "--compact", "-A", "0.2", "-p", "50"])
    assert (d / "a.uvdb").read_bytes() == (d / "b.uvdb").read_bytes()
    dev, host = _routes(err)
    assert dev == 0 and host == CL.CompactFile(d / "a.uvdb").n_tiles > 4


def test_search_over_the_device_encoded_file_and_the_dense_one(aligned):
    d, _ = aligned
    path, err = _align_compact(d, "search", ["-p", "1000"])
    assert _routes(err)[0] > 0
    names, rows = F.read_fasta_bytes(_xz(d / "t.aln.xz"))
    _write_fasta(d / "queries.fa", ["query %d" % i for i in range(6)], [rows[i] for i in (0, 9, 500, 4200, 4350, len(rows) - 1)])
    tables = []
    for tag, db in (("c", path), ("d", d / "dense.uvdb")):
        out = str(d / ("nn_" + tag))
        _run([UVAIA, "--packed", str(db), str(d / "queries.fa"), "-A", AMBIG_R, "-n", "6", "-o", out])
        tables.append((_xz(out + ".csv.xz"), _xz(out + ".aln.xz")))
    assert tables[0] == tables[1] and len(tables[0][0].splitlines()) > 12


CLUST = ["-d", "1", "-p", "64"]


@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    """4 400 aligned rows of 320 sites with 14 private substitutions each: at -d 1 nearly every one stays a medoid"""
    d = tmp_path_factory.mktemp("encode_clust")
    rows = _lineage(N_SEQ, 320, 61, private=14)
    _write_fasta(d / "in.fa", ["s%d" % i for i in range(N_SEQ)], rows)
    _run([UVAIAPACK, "-A", "1", "-o", str(d / "in.uvdb"), str(d / "in.fa")])
    env = dict(os.environ, OMP_NUM_THREADS="8")
    return d, env


@pytest.mark.parametrize("source", ["text", "packed"])
@pytest.mark.parametrize("keep", [[], ["--keep-medoids"]])
def test_uvaiaclust_compact_is_uvaiapack_compact_of_its_alignment(clustered, source, keep):
    d, env = clustered
    tag = source + ("_keep" if keep else "")
    inp = [str(d / "in.fa")] if source == "text" else ["--packed", str(d / "in.uvdb")]
    err = _run([UVAIACLUST] + CLUST + keep + inp + ["--packed-out", str(d / (tag + ".uvdb")), "--compact", "-A", "0.5", "-o", str(d / tag)], env)
    names, rows = F.read_fasta_bytes(_xz(d / (tag + ".aln.xz")))
    kept = [r for r in rows if R.count_non_n(r) >= int(len(rows[0]) * 0.5)]
    assert len(kept) > 4096 + 64                                                   # more than 4 160 medoids remain: a whole tile behind the sample
    _run([UVAIAPACK, "-A", "0.5", "--compact", "-o", str(d / (tag + "_ref.uvdb")), str(d / (tag + ".aln.xz"))])
    assert (d / (tag + ".uvdb")).read_bytes() == (d / (tag + "_ref.uvdb")).read_bytes()
    dev, host = _routes(err)
    assert dev > 0 and dev + host == (len(kept) + 63) // 64


@pytest.fixture(scope="module")
def packed_rows(tmp_path_factory):
    """4 400 rows and the compact file the host writer makes of packed_lib's tiles of them"""
    d = tmp_path_factory.mktemp("encode_pack")
    rows = _lineage(N_SEQ, 330, 71, private=3)
    names = ["row%d" % i for i in range(N_SEQ)]
    planes, non_n = P.pack_tiles(rows, 330)
    CL.write_compact(d / "host.uvdb", names, rows, planes, non_n)
    _write_fasta(d / "all.fa", names, rows)
    _write_fasta(d / "h1.fa", names[:2210], rows[:2210])
    _write_fasta(d / "h2.fa", names[2210:], rows[2210:])
    return d


def test_uvaiapack_compact_is_the_host_writers_file(packed_rows):
    d = packed_rows
    err = _run([UVAIAPACK, "--compact", "-o", str(d / "cli.uvdb"), str(d / "all.fa")])
    assert (d / "cli.uvdb").read_bytes() == (d / "host.uvdb").read_bytes()
    assert "Packed %d of %d" % (N_SEQ, N_SEQ) in err


def test_uvaiapack_merge_compact_of_two_halves_is_the_host_writers_file(packed_rows):
    d = packed_rows
    _run([UVAIAPACK, "-o", str(d / "h1.uvdb"), str(d / "h1.fa")])
    _run([UVAIAPACK, "--compact", "-o", str(d / "h2.uvdb"), str(d / "h2.fa")])
    err = _run([UVAIAPACK, "--merge", "--compact", "-o", str(d / "merged.uvdb"), str(d / "h1.uvdb"), str(d / "h2.uvdb")])
    assert (d / "merged.uvdb").read_bytes() == (d / "host.uvdb").read_bytes()
    assert "Merged %d of %d" % (N_SEQ, N_SEQ) in err
