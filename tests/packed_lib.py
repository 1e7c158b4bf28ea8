"""Helpers of the packed-database tests: the interchange tiles restated in numpy (no GPU needed) and a ctypes view of the
host library's uvdb writer and reader (uvaia_amd/csrc/host/uvdb.h)."""
import ctypes as C

import numpy as np

from uvaia_amd import hostlib

CODE = b"NACMGRSVTWYHKDBN"          # character of a set of bases, bit 0 = A, 1 = C, 2 = G, 3 = T (empty and full set: N)
EXCEPTIONS = b"-?XO."               # invalid characters the planes cannot tell from N: the file's exception runs
SIDE_ROW_INTS = 64


def _lut():
    lut = np.zeros(256, dtype=np.uint8)
    for code, ch in enumerate(CODE[1:15], 1):
        lut[ch] = code
        lut[ch + 32] = code         # lower case
    return lut


def tile_bytes(nchar):
    return ((nchar + 31) // 32 + 3) // 4 * 4 * 64 * 16


def pack_tiles(seqs, nchar):
    """(planes uint8 [n_tiles, tile_bytes], non_n int32 [n_tiles * 64]): tile[word group][plane A,C,G,T][lane] 16-byte words,
    bit s of word w = site 32 w + s; lanes past the last sequence are zero."""
    n, W4 = len(seqs), ((nchar + 31) // 32 + 3) // 4
    n_tiles = (n + 63) // 64
    codes = np.zeros((n_tiles * 64, W4 * 128), dtype=np.uint8)
    lut = _lut()
    for i, s in enumerate(seqs):
        codes[i, :nchar] = lut[np.frombuffer(s, dtype=np.uint8)]
    out = np.zeros((n_tiles, W4, 4, 64, 4), dtype=np.uint32)
    weights = (np.uint32(1) << np.arange(32, dtype=np.uint32))
    for p in range(4):
        bits = ((codes >> p) & 1).astype(np.uint32).reshape(n_tiles, 64, W4, 4, 32)
        words = (bits * weights).sum(axis=4, dtype=np.uint64).astype(np.uint32)          # [tile, lane, w4, j]
        out[:, :, p, :, :] = words.transpose(0, 2, 1, 3)
    non_n = (codes != 0).sum(axis=1).astype(np.int32)
    return out.view(np.uint8).reshape(n_tiles, tile_bytes(nchar)), non_n


def decode_reference(planes, i, nchar):
    """text of reference i as the planes alone give it (every invalid site reads N)"""
    W4 = ((nchar + 31) // 32 + 3) // 4
    t = planes.reshape(-1).view(np.uint32).reshape(-1, W4, 4, 64, 4)[i // 64, :, :, i % 64, :]      # [w4, plane, j]
    sets = np.zeros(W4 * 128, dtype=np.uint8)
    for p in range(4):
        words = t[:, p, :].reshape(-1)
        bits = (words[:, None] >> np.arange(32, dtype=np.uint32)) & 1
        sets |= (bits.reshape(-1).astype(np.uint8) << p)
    return np.frombuffer(CODE, dtype=np.uint8)[sets[:nchar]].tobytes()


def _lib():
    L = hostlib.load_library()
    if not getattr(L, "_uvdb_ready", False):
        L.uvdb_create.restype = C.c_void_p
        L.uvdb_create.argtypes = [C.c_char_p, C.c_int, C.c_size_t, C.c_int, C.c_double]
        L.uvdb_add_reference.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.uvdb_add_tiles.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.uvdb_close.argtypes = [C.c_void_p]
        L.uvdb_open.restype = C.c_void_p
        L.uvdb_open.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        L.uvdb_unpack_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p]
        L.uvdb_unpack_reference.restype = None
        L.uvdb_apply_exceptions.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p]
        L.uvdb_apply_exceptions.restype = None
        L.uvdb_close_reader.argtypes = [C.c_void_p]
        L.uvdb_close_reader.restype = None
        L.uvdb_radius_filter_is_exact.argtypes = [C.c_int, C.c_double, C.c_double]
        L.uvdb_radius_filter_is_exact.restype = C.c_int
        L._uvdb_ready = True
    return L


def write_uvdb(path, names, seqs, planes, non_n, side_rows=None, ref_ambiguity=0.5):
    """seqs: upper-case text (what the FASTA reader hands to uvaiapack); planes / non_n / side_rows in the engine's export form"""
    L = _lib()
    nchar = len(seqs[0])
    n_tiles = (len(seqs) + 63) // 64
    planes = np.ascontiguousarray(planes, dtype=np.uint8)
    non_n = np.ascontiguousarray(non_n, dtype=np.int32)
    side = np.zeros((n_tiles * 64, SIDE_ROW_INTS), dtype=np.int32) if side_rows is None else np.ascontiguousarray(side_rows, dtype=np.int32)
    w = L.uvdb_create(str(path).encode(), nchar, tile_bytes(nchar), SIDE_ROW_INTS, ref_ambiguity)
    assert w
    for nm, s in zip(names, seqs):
        assert L.uvdb_add_reference(w, nm.encode(), s) == 0
    assert L.uvdb_add_tiles(w, n_tiles, planes.ctypes.data, non_n.ctypes.data, side.ctypes.data) == 0
    assert L.uvdb_close(w) == 0


class Reader:
    def __init__(self, path, nchar):
        self.L = _lib()
        err = C.create_string_buffer(512)
        self.r = self.L.uvdb_open(str(path).encode(), err, 512)
        assert self.r, err.value
        self.nchar = nchar

    def unpack_reference(self, i):
        out = C.create_string_buffer(self.nchar + 1)
        self.L.uvdb_unpack_reference(self.r, i, out)
        return out.raw[:self.nchar]

    def apply_exceptions(self, i, row):
        buf = C.create_string_buffer(bytes(row), self.nchar + 1)
        self.L.uvdb_apply_exceptions(self.r, i, buf)
        return buf.raw[:self.nchar]

    def close(self):
        if self.r:
            self.L.uvdb_close_reader(self.r)
            self.r = None


def radius_filter_is_exact(nchar, ball_ambiguity, pack_ambiguity):
    return int(_lib().uvdb_radius_filter_is_exact(int(nchar), float(ball_ambiguity), float(pack_ambiguity)))


def awkward_references(n, nchar, seed):
    """references that hold every IUPAC code, N runs, '-', '?', '.', 'X', 'O' and lower-case letters"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTacgtMRWSYKVHDBmrwsykvhdbNn", dtype=np.uint8)
    out = []
    for i in range(n):
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar)
        pos = rng.choice(nchar, size=nchar // 6, replace=False)
        s[pos] = rng.choice(alphabet, size=len(pos))
        for ch in b"N-?.XO":
            for _ in range(2):
                a = int(rng.integers(0, nchar))
                s[a:a + int(rng.integers(1, 40))] = ch
        if i % 3 == 0:
            s[:int(rng.integers(1, 70))] = ord("N")           # leading and trailing runs, across word boundaries
            s[nchar - int(rng.integers(1, 70)):] = ord("-")
        s[(i * 7) % nchar] = alphabet[i % len(alphabet)]      # every letter of the alphabet somewhere in the set
        out.append(s.tobytes())
    return out
