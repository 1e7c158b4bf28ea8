"""The windowed search over a packed database (`uvaia --packed --window`), on a GPU box: staged tiles, the selection of their lanes into
the resident store (select_tiles_kernel), the search window after window against one resident search of the same stream and against the
oracle, the text of a loaded window, and the command against itself without --window."""
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import fixtures as F
import oracle_lib as O
import packed_lib as P
from uvaia_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIA = os.path.join(ROOT, "bin", "uvaia")
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")
N_REF = 700
_cache = {}


def _cut(bundled_db, nchar):
    """700 references and 40 queries of the bundled alignment on nchar of its columns, spread over the genome (without its ends)"""
    if nchar not in _cache:
        names, seqs = bundled_db
        cols = np.linspace(400, 29400, nchar).astype(np.int64)
        pick = lambda s: np.frombuffer(s, dtype=np.uint8)[cols].tobytes()
        refs = [pick(s) for s in seqs[:N_REF]]
        qs = [pick(s) for s in seqs[1000:1040]]
        qn = list(names[1000:1040])
        with capi.Engine.from_query(O.Query(qs[:5], qn[:5]), nbest=2, max_pool=64) as eng:       # the interchange tiles, out of a default-mode context
            eng.db_reserve(len(refs))
            eng.db_append(refs)
            tiles = eng.db_export()
        _cache[nchar] = (list(names[:N_REF]), refs, qn, qs, tiles)
    return _cache[nchar]


def _awkward_set(nchar, n, seed):
    """five queries, n references that hold every IUPAC code and every exception character (so that side rows are not empty), their
    upper-case text and their interchange tiles out of a default-mode context"""
    key = ("awkward", nchar, n, seed)
    if key not in _cache:
        root = F.random_acgt(nchar, 11)
        qs = []
        for i in range(5):
            s = bytearray(root)
            s[17 * i + 3] = b"ACGT"[(b"ACGT".index(s[17 * i + 3]) + 1) % 4]
            qs.append(bytes(s))
        qn = ["q%d" % i for i in range(len(qs))]
        refs = P.awkward_references(n, nchar, seed=seed)
        with capi.Engine.from_query(O.Query(qs, qn), nbest=2, max_pool=64) as eng:
            eng.db_reserve(len(refs))
            eng.db_append(refs)
            tiles = eng.db_export()
        _cache[key] = (qs, qn, [r.upper() for r in refs], tiles)
    return _cache[key]


def _windowed(eng, tiles, n, window, pool, stage_first=True, keep=None):
    """the loop of the command: window after window of the kept stream (keep: file positions, None = all), the next one staged before or
    after the current one is searched; the concatenated entered flags"""
    planes, non_n, side = tiles
    keep = np.arange(n) if keep is None else np.asarray(keep)
    spans = []
    for a in range(0, len(keep), window):
        b = min(len(keep), a + window)
        t0, t1 = int(keep[a]) // 64, int(keep[b - 1]) // 64 + 1
        spans.append((a, b, t0, t1 - t0, (keep[a:b] - t0 * 64).astype(np.int32)))
    eng.db_stage_reserve(max(s[3] for s in spans))
    stage = lambda w: eng.db_stage_packed(w & 1, planes[spans[w][2]:spans[w][2] + spans[w][3]], non_n[spans[w][2] * 64:(spans[w][2] + spans[w][3]) * 64],
                                          side[spans[w][2] * 64:(spans[w][2] + spans[w][3]) * 64], spans[w][3])
    stage(0)
    entered, loads = [], []
    for w, (a, b, t0, nt, sel) in enumerate(spans):
        identity = np.array_equal(sel, np.arange(b - a))
        eng.db_load_staged(w & 1, None if identity else sel, b - a)
        assert eng.db_size() == b - a
        loads.append(b - a)
        if stage_first and w + 1 < len(spans):
            stage(w + 1)
        entered.append(eng.search_resident(pool, ordinal0=a))
        if not stage_first and w + 1 < len(spans):
            stage(w + 1)
    return np.concatenate(entered), loads


def _same_drain(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- API parity
@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("nq", [5, 40])
@pytest.mark.parametrize("nchar", [128, 129, 331])
def test_windows_give_the_heaps_of_one_resident_search(bundled_db, nchar, nq, acgt):
    rnames, refs, qn, qs, tiles = _cut(bundled_db, nchar)
    q = O.Query(qs[:nq], qn[:nq], acgt=acgt)
    assert len(q.idx_c) > 0                                  # constant-and-complete columns: pool boundaries matter
    with capi.Engine.from_query(q, nbest=4, max_pool=128) as eng:
        assert eng.scan_variant() == (0 if nq == 5 else 2)   # the two-counter scan over packed planes; the column-compressed one (planes derived per load)
        results = {}
        for pool, window in ((128, 256), (96, 192)):
            eng.reset(); eng.db_clear()
            eng.db_append_packed(*tiles, N_REF)
            ent = eng.search_resident(pool)
            want = eng.drain()
            results[pool] = (want, ent)
            for stage_first in (True, False):
                eng.reset()
                got_ent, loads = _windowed(eng, tiles, N_REF, window, pool, stage_first)
                got = eng.drain()
                assert loads[-1] == N_REF % window and loads[-1] % 64 != 0 and len(loads) == -(-N_REF // window)
                assert _same_drain(got, want), (nchar, nq, acgt, pool, stage_first)          # heaps, ordinals and max_incompatible
                assert np.array_equal(got_ent, ent), (nchar, nq, acgt, pool, stage_first)
        if nchar == 331 and nq == 40:                        # once per mode: and they are the oracle's
            (n, T, sc, od), ent = results[128]
            gold = O.search(q, refs, rnames, pool=128, nbest=4, ambig_r=0.999)
            got = capi.finalise_heaps(n, sc, od)
            for iq in range(q.ntax):
                assert got[iq] == [(tuple(s), o) for o, _, s in gold.rows[iq]], iq
            assert list(T) == gold.final_T
            assert np.array_equal(np.nonzero(ent)[0], gold.saved)


# ---------------------------------------------------------------------------------------------------------------- selection
# kept positions of four staged tiles: holes at lane 0 of tiles 0 and 1 (and more), the whole of tile 2, the last staged lane
SEL = list(range(1, 21)) + list(range(65, 85)) + list(range(192, 255))


def _compact(tiles, sel):
    """host-side compaction of the same lanes: (planes, non_n, side rows) of ceil(len(sel) / 64) tiles, zero past the last"""
    planes, non_n, side = tiles
    nt = (len(sel) + 63) // 64
    src = planes.reshape(planes.shape[0], -1, 64, 16)        # [tile][word group x plane][lane][16 bytes]
    out = np.zeros((nt,) + src.shape[1:], dtype=np.uint8)
    out_n = np.zeros(nt * 64, dtype=np.int32)
    out_s = np.zeros((nt * 64, side.shape[1]), dtype=np.int32)
    for k, s in enumerate(sel):
        out[k // 64, :, k % 64, :] = src[s // 64, :, s % 64, :]
        out_n[k] = non_n[s]
        out_s[k] = side[s]
    return out.reshape(nt, -1), out_n, out_s


@pytest.mark.parametrize("n_ref", [1, 64, 65, len(SEL)])
def test_load_staged_is_the_host_side_compaction(n_ref):
    qs, qn, upper, tiles = _awkward_set(129, 256, 7)
    assert tiles[2][:, 0].max() > 0                          # the side rows are not empty
    with capi.Engine.from_query(O.Query(qs, qn), nbest=4, max_pool=128) as eng:
        eng.db_append_packed(*tiles, 256)                    # something larger is resident before: its lanes must not show through
        eng.db_stage_reserve(4)
        eng.db_stage_packed(1, tiles[0][:4], tiles[1][:256], tiles[2][:256], 4)
        sel = SEL[:n_ref]
        eng.db_load_staged(1, sel, n_ref)
        assert eng.db_size() == n_ref
        want = _compact(tiles, sel)
        got = eng.db_export()
        for g, w in zip(got, want):
            assert np.array_equal(g, w), n_ref
        # a selection entry outside the staged tiles: refused, the database and the heaps as before
        eng.search_resident(64)
        state = eng.drain()
        for bad in ([-1], sel[:-1] + [256], [0, 1 << 30]):
            with pytest.raises(capi.GpuError) as ei:
                eng.db_load_staged(1, bad, len(bad))
            assert ei.value.code == -1
        with pytest.raises(capi.GpuError) as ei:             # and a slot that does not exist
            eng.db_load_staged(2, None, 1)
        assert ei.value.code == -1
        assert eng.db_size() == n_ref
        assert all(np.array_equal(g, w) for g, w in zip(eng.db_export(), want))
        assert _same_drain(eng.drain(), state)
        eng.db_load_staged(1, None, 200)                     # the identity selection, a last tile of 8
        assert all(np.array_equal(g, w) for g, w in zip(eng.db_export(), _compact(tiles, list(range(200)))))


# ---------------------------------------------------------------------------------------------------------------- decode
NCHAR = 333                                                  # not a multiple of 16, 32 or 128


@pytest.fixture(scope="module")
def awkward(tmp_path_factory):
    d = tmp_path_factory.mktemp("window_unpack")
    qs, qn, upper, tiles = _awkward_set(NCHAR, 150, 23)      # three tiles, 22 references in the last
    P.write_uvdb(d / "awkward.uvdb", ["r%d" % i for i in range(len(upper))], upper, *tiles)
    return qs, qn, upper, tiles, P.Reader(d / "awkward.uvdb", NCHAR)


@pytest.mark.parametrize("pitch", [NCHAR, (NCHAR + 15) // 16 * 16])
@pytest.mark.parametrize("acgt", [False, True])
def test_text_of_a_loaded_window(awkward, acgt, pitch):
    qs, qn, upper, tiles, reader = awkward
    n = len(upper)
    with capi.Engine.from_query(O.Query(qs, qn, acgt=acgt), nbest=2, max_pool=256) as eng:
        with pytest.raises(capi.GpuError) as ei:             # no window yet
            eng.db_unpack_rows([0], pitch)
        assert ei.value.code == -6
        eng.db_stage_reserve(3)
        eng.db_stage_packed(0, *tiles, 3)
        kept = [i for i in range(n) if i not in (0, 64, 149)]
        for sel in (None, kept):
            pos = list(range(n)) if sel is None else sel
            eng.db_load_staged(0, sel, len(pos))
            for index in (list(range(len(pos))), list(range(len(pos) - 1, -1, -1)), [5, 5, 0, len(pos) - 1, 64, 63]):
                rows = eng.db_unpack_rows(index, pitch)
                assert len(rows) == len(index)
                for k, row in zip(index, rows):
                    assert reader.apply_exceptions(pos[k], row) == reader.unpack_reference(pos[k]) == upper[pos[k]], (acgt, k)
            for bad in ([len(pos)], [0, -1], [3, 1 << 20]):  # outside the window: an error code, not a fault
                with pytest.raises(capi.GpuError) as ei:
                    eng.db_unpack_rows(bad, pitch)
                assert ei.value.code == -1
            assert eng.db_unpack_rows([len(pos) - 1], pitch)[0] == P.decode_reference(tiles[0], pos[-1], NCHAR)     # ... and the context is still usable
        with pytest.raises(capi.GpuError) as ei:             # the entry of the radius search keeps its behaviour and its text
            eng.unpack_rows([0])
        assert ei.value.code == -6 and "no packed batch to unpack: uvaia_gpu_ball_packed comes first" in str(ei.value)
        ms = eng.window_ms(reset=True)
        assert ms[0] > 0 and ms[2] > 0 and eng.window_ms() == (0.0, 0.0, 0.0)
        assert eng.free_bytes() > 0


# ---------------------------------------------------------------------------------------------------------------- command
def _write_fasta(path, names, seqs):
    with open(path, "wb") as fh:
        for n, s in zip(names, seqs):
            fh.write(b">" + n.encode() + b"\n" + s + b"\n")


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return r.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def files(tmp_path_factory, bundled_db):
    d = tmp_path_factory.mktemp("window_cli")
    rnames, refs, qn, qs, tiles = _cut(bundled_db, 331)
    _write_fasta(d / "refs.fa", rnames, refs)
    _run([UVAIAPACK, "-A", "0.999", "-o", str(d / "db.uvdb"), str(d / "refs.fa")])
    same = [0, 64] + list(range(128, 192)) + [N_REF - 1]     # queries named like references: lane 0 of tiles, a whole tile, the last one
    _write_fasta(d / "q.fa", [rnames[i] for i in same], [refs[i] for i in same])
    return d, len(same)


def _counts(log):
    return (re.search(r"Loaded (\d+) packed sequences", log).group(1), re.search(r"Total of (\d+) sequences searched; (\d+) saved", log).groups(),
            re.search(r"Saved (\d+) sequences to file", log).group(1), re.findall(r" (\d+) reference sequences already present", log))


@pytest.mark.parametrize("acgt", [[], ["--acgt"]])
@pytest.mark.parametrize("exclude", [[], ["-x"]])
def test_uvaia_window_writes_the_files_of_the_resident_command(files, exclude, acgt):
    d, n_same = files
    tag = "".join(x.strip("-") for x in exclude + acgt)
    out_r, out_w = str(d / ("r_" + tag)), str(d / ("w_" + tag))
    base = [UVAIA, "--packed", str(d / "db.uvdb"), str(d / "q.fa"), "-n", "4", "-p", "128", "-A", "0.999"] + exclude + acgt
    log_r = _run(base + ["-o", out_r])
    log_w = _run(base + ["-o", out_w, "--window", "256", "--window-report"])
    for suffix in (".csv.xz", ".aln.xz"):
        text = lzma.open(out_r + suffix, "rb").read()
        assert lzma.open(out_w + suffix, "rb").read() == text, suffix
        assert len(text) > 1000
    assert _counts(log_w) == _counts(log_r)
    loaded = int(_counts(log_r)[0])
    assert loaded == N_REF - (n_same if exclude else 0)
    report = re.search(r'window report: \{"window": (\d+), "n_windows": (\d+)', log_w)
    assert report and int(report.group(1)) == 256 and int(report.group(2)) == -(-loaded // 256) >= 3
    assert "window report" not in log_r
