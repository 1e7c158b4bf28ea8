"""Helpers of the compact packed-database tests (version 2 of uvaia_amd/csrc/host/uvdb.h): ctypes views of the compact writer, the reader and
uvdb_expand_tiles, the file's sections read with numpy, and the side rows' fixed form restated in numpy.  The dense tiles and the awkward
references come from packed_lib."""
import ctypes as C

import numpy as np

import packed_lib as PL

BASE_SAMPLE = 4096
MAX_NCHAR = 2097152
HEAD_MAX_WORDS = 2047
SIDE_LISTED = 11


def _lib():
    L = PL._lib()
    if not getattr(L, "_uvdb_compact_ready", False):
        L.uvdb_create_compact.restype = C.c_void_p
        L.uvdb_create_compact.argtypes = [C.c_char_p, C.c_int, C.c_size_t, C.c_int, C.c_double]
        L.uvdb_expand_tiles.restype = C.c_int
        L.uvdb_expand_tiles.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.uvdb_tile_planes.restype = C.c_void_p
        L.uvdb_tile_planes.argtypes = [C.c_void_p, C.c_uint64]
        L.uvdb_tile_side_rows.restype = C.c_void_p
        L.uvdb_tile_side_rows.argtypes = [C.c_void_p, C.c_uint64]
        L.uvdb_file_version.restype = C.c_uint32
        L.uvdb_file_version.argtypes = [C.c_char_p]
        L._uvdb_compact_ready = True
    return L


def n_words(nchar):
    return ((nchar + 31) // 32 + 3) // 4 * 4


def create_compact(path, nchar, tile_bytes=None):
    """the writer handle (None: refused)"""
    return _lib().uvdb_create_compact(str(path).encode(), int(nchar), PL.tile_bytes(nchar) if tile_bytes is None else tile_bytes, PL.SIDE_ROW_INTS, 0.5)


def write_compact(path, names, seqs, planes, non_n, ref_ambiguity=0.5, chunk_tiles=None):
    """as packed_lib.write_uvdb, through uvdb_create_compact; chunk_tiles: tiles per uvdb_add_tiles call (None: all at once)"""
    L = _lib()
    nchar = len(seqs[0])
    n_tiles = (len(seqs) + 63) // 64
    planes = np.ascontiguousarray(planes, dtype=np.uint8).reshape(n_tiles, PL.tile_bytes(nchar))
    non_n = np.ascontiguousarray(non_n, dtype=np.int32)
    w = L.uvdb_create_compact(str(path).encode(), nchar, PL.tile_bytes(nchar), PL.SIDE_ROW_INTS, ref_ambiguity)
    assert w
    step = n_tiles if not chunk_tiles else chunk_tiles
    for t in range(0, max(n_tiles, 1), max(step, 1)):
        e = min(n_tiles, t + step)
        for nm, s in zip(names[t * 64:e * 64], seqs[t * 64:e * 64]):           # named first, then their tiles, as the commands do
            assert L.uvdb_add_reference(w, nm.encode(), s) == 0
        p, nn = np.ascontiguousarray(planes[t:e]), np.ascontiguousarray(non_n[t * 64:e * 64])
        assert L.uvdb_add_tiles(w, e - t, p.ctypes.data, nn.ctypes.data, None) == 0
    assert L.uvdb_close(w) == 0


class CompactFile:
    """the sections of a version 2 file, read with numpy (copies: a test may damage the bytes it took them from)"""
    OFF = {"off_base": 56, "off_nonn": 64, "off_head_idx": 72, "off_name_idx": 80, "off_names": 88, "off_exc_idx": 96, "off_exc": 104, "file_bytes": 112,
           "off_heads": 120, "off_lit_idx": 128}

    def __init__(self, path):
        raw = np.fromfile(str(path), dtype=np.uint8)
        self.raw = raw
        u32 = lambda o: int(raw[o:o + 4].view(np.uint32)[0])
        u64 = lambda o: int(raw[o:o + 8].view(np.uint64)[0])
        self.version, self.nchar, self.W4 = u32(8), u32(12), u32(16)
        self.n_ref, self.n_tiles, self.tile_bytes = u64(24), u64(32), u64(40)
        for k, o in self.OFF.items():
            setattr(self, k, u64(o))
        lanes = self.n_tiles * 64
        self.lanes = lanes
        self.off_lits = (self.off_lit_idx + (lanes + 1) * 8 + 63) // 64 * 64
        self.base = raw[self.off_base:self.off_base + self.W4 * 64].view(np.uint32).copy()             # [W4][plane][4]
        self.non_n = raw[self.off_nonn:self.off_nonn + lanes * 4].view(np.int32).copy()
        self.head_idx = raw[self.off_head_idx:self.off_head_idx + (lanes + 1) * 8].view(np.uint64).copy()
        self.lit_idx = raw[self.off_lit_idx:self.off_lit_idx + (lanes + 1) * 8].view(np.uint64).copy()
        nh, nl = int(self.head_idx[-1]), int(self.lit_idx[-1])
        self.heads = raw[self.off_heads:self.off_heads + nh * 4].view(np.uint32).copy()
        self.lits = raw[self.off_lits:self.off_lits + nl * 16].view(np.uint32).copy()

    def heads_of(self, i):
        """[(first_word, n_words, literal, code)] of lane i"""
        out = []
        for h in self.heads[int(self.head_idx[i]):int(self.head_idx[i + 1])]:
            h = int(h)
            out.append((h >> 16, (h >> 5) & 0x7FF, (h >> 4) & 1, h & 15))
        return out

    def base_word(self, w):
        """planes A, C, G, T of word w of the base"""
        b = self.base.reshape(self.W4, 4, 4)
        return tuple(int(b[w // 4, p, w % 4]) for p in range(4))

    def stage_args(self, t0, nt):
        """what Engine.db_stage_compact_at takes for tiles t0 .. t0 + nt - 1"""
        return (self.base, self.head_idx[t0 * 64:(t0 + nt) * 64 + 1], self.heads, self.lit_idx[t0 * 64:(t0 + nt) * 64 + 1], self.lits,
                self.non_n[t0 * 64:(t0 + nt) * 64], nt)


def head(first, n, literal, code):
    return (first << 16) | (n << 5) | (literal << 4) | code


def try_open(path):
    """(opened?, message) of uvdb_open"""
    L = _lib()
    err = C.create_string_buffer(512)
    r = L.uvdb_open(str(path).encode(), err, 512)
    if r:
        L.uvdb_close_reader(r)
    return bool(r), err.value.decode()


class Reader(PL.Reader):
    def __init__(self, path, nchar):
        _lib()
        super().__init__(path, nchar)

    def expand_tiles(self, first_tile, n_tiles, side=True):
        """(planes uint8 [n_tiles, tile_bytes], side rows int32 [n_tiles * 64, 64]) of uvdb_expand_tiles"""
        planes = np.full((n_tiles, PL.tile_bytes(self.nchar)), 0xA5, dtype=np.uint8)
        rows = np.full((n_tiles * 64, PL.SIDE_ROW_INTS), -7, dtype=np.int32)
        assert self.L.uvdb_expand_tiles(self.r, first_tile, n_tiles, planes.ctypes.data, rows.ctypes.data if side else None) == 0
        return planes, rows

    def dense_pointers_are_null(self):
        return self.L.uvdb_tile_planes(self.r, 0) is None and self.L.uvdb_tile_side_rows(self.r, 0) is None


def file_version(path):
    return int(_lib().uvdb_file_version(str(path).encode()))


def side_rows_canonical(planes, nchar):
    """the side rows as the engine's export fixes them, from dense tiles: per reference the words with a partially ambiguous site (two
    planes set at one site) in ascending order; [0] their number, [1..11] the first eleven, [12 + 4k + p] plane p of the k-th listed"""
    W4 = n_words(nchar) // 4
    t = np.ascontiguousarray(planes).reshape(-1).view(np.uint32).reshape(-1, W4, 4, 64, 4)
    n_tiles = t.shape[0]
    w = t.transpose(0, 3, 1, 4, 2).reshape(n_tiles * 64, W4 * 4, 4)                # [lane, word, plane]
    a, c, g, tt = w[:, :, 0], w[:, :, 1], w[:, :, 2], w[:, :, 3]
    amb = ((a & c) | (a & g) | (a & tt) | (c & g) | (c & tt) | (g & tt)) != 0
    rows = np.zeros((n_tiles * 64, PL.SIDE_ROW_INTS), dtype=np.int32)
    for i in range(n_tiles * 64):
        ws = np.flatnonzero(amb[i])
        rows[i, 0] = len(ws)
        for k, word in enumerate(ws[:SIDE_LISTED]):
            rows[i, 1 + k] = word
            rows[i, 12 + 4 * k:16 + 4 * k] = w[i, word].view(np.int32)
    return rows


def near_identical_references(n, nchar, seed):
    """genomes of one lineage: one random ACGT row, every reference a copy with a few substitutions, an IUPAC code now and then, a
    leading and a trailing N run and sometimes a gap"""
    rng = np.random.default_rng(seed)
    root = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar)
    out = []
    for i in range(n):
        s = root.copy()
        k = int(rng.integers(0, 4))
        if k:
            s[rng.choice(nchar, size=min(k, nchar), replace=False)] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=min(k, nchar))
        if i % 5 == 1:
            s[int(rng.integers(0, nchar))] = rng.choice(np.frombuffer(b"RYKM", dtype=np.uint8))
        if i % 2:
            s[:int(rng.integers(0, min(nchar, 80)))] = ord("N")
            s[nchar - int(rng.integers(0, min(nchar, 80))):] = ord("N")
        if i % 7 == 3:
            a = int(rng.integers(0, nchar))
            s[a:a + int(rng.integers(1, 50))] = ord("-")
        out.append(s.tobytes())
    return out
