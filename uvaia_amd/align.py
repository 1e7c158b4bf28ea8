"""ctypes binding of include/uvaia_align.h (tests and bench.py reach the wavefront aligner of `uvaialign` through it)."""
import ctypes as C

import numpy as np

from . import capi

# every symbol include/uvaia_align.h declares (tests check the library exports all of them)
SYMBOLS = [
    "uvaia_align_default_options", "uvaia_align_open", "uvaia_align_close", "uvaia_align_last_error", "uvaia_align_batch",
    "uvaia_align_load", "uvaia_align_load_block", "uvaia_align_run", "uvaia_align_sync", "uvaia_align_fetch", "uvaia_align_stats",
    "uvaia_align_device_rows", "uvaia_align_load_device", "uvaia_align_set_insertions", "uvaia_align_insertion_counts",
    "uvaia_align_fetch_insertions", "uvaia_align_set_variants", "uvaia_align_variant_counts", "uvaia_align_fetch_variants",
    "uvaia_align_variants_of", "uvaia_align_variants_ms",
]

# uvaia_align_variant and uvaia_align_row_qc as numpy sees them
VARIANT_DTYPE = np.dtype([("query", "<i4"), ("ref_pos", "<i4"), ("length", "<i4"), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"), ("pad", "u1")])
QC_DTYPE = np.dtype([(k, "<i4") for k in ("matches", "substitutions", "deletion_runs", "deleted_sites", "unknown_sites", "other_sites", "first_site", "last_site")])


class AlignError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("uvaia_align error %d: %s" % (code, msg))
        self.code = code


class Options(C.Structure):
    _fields_ = [("mismatch", C.c_int), ("gap_opening", C.c_int), ("gap_extension", C.c_int), ("min_wavefront_length", C.c_int),
                ("max_distance_threshold", C.c_int), ("workspace_bytes", C.c_size_t), ("max_blocks", C.c_int)]


class Insertion(C.Structure):
    _fields_ = [("query", C.c_int), ("ref_pos", C.c_int), ("seq_pos", C.c_int), ("length", C.c_int)]


_ready = False


def _lib():
    global _ready
    L = capi.load_library()
    if not _ready:
        vp, pi = C.c_void_p, C.POINTER(C.c_int)
        L.uvaia_align_default_options.argtypes = [C.POINTER(Options)]
        L.uvaia_align_default_options.restype = None
        L.uvaia_align_open.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int, C.c_int, C.POINTER(Options)]
        L.uvaia_align_close.argtypes = [vp]
        L.uvaia_align_close.restype = None
        L.uvaia_align_last_error.argtypes = [vp]
        L.uvaia_align_last_error.restype = C.c_char_p
        L.uvaia_align_batch.argtypes = [vp, C.POINTER(C.c_char_p), pi, C.c_int, C.c_void_p, pi]
        L.uvaia_align_load.argtypes = [vp, C.POINTER(C.c_char_p), pi, C.c_int]
        L.uvaia_align_load_block.argtypes = [vp, C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        L.uvaia_align_load_device.argtypes = [vp, C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        L.uvaia_align_run.argtypes = [vp]
        L.uvaia_align_sync.argtypes = [vp]
        L.uvaia_align_fetch.argtypes = [vp, C.c_void_p, pi]
        L.uvaia_align_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_double), pi, C.POINTER(C.c_double)]
        L.uvaia_align_device_rows.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), pi, pi]
        L.uvaia_align_set_insertions.argtypes = [vp, C.c_int, C.c_size_t]
        L.uvaia_align_insertion_counts.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.uvaia_align_fetch_insertions.argtypes = [vp, C.c_void_p, C.c_void_p]
        L.uvaia_align_set_variants.argtypes = [vp, C.c_int]
        L.uvaia_align_variant_counts.argtypes = [vp, C.POINTER(C.c_longlong), pi]
        L.uvaia_align_fetch_variants.argtypes = [vp, C.c_void_p, C.c_void_p]
        L.uvaia_align_variants_of.argtypes = [vp, C.c_void_p, C.c_size_t, C.c_int]
        L.uvaia_align_variants_ms.argtypes = [vp, C.c_int]
        L.uvaia_align_variants_ms.restype = C.c_double
        _ready = True
    return L


def default_options():
    o = Options()
    _lib().uvaia_align_default_options(C.byref(o))
    return o


class Aligner:
    """One reference sequence on one GPU (new_queue, src/align.c:286-313)."""

    def __init__(self, ref, device=0, **options):
        self.L = _lib()
        self.ref_len = len(ref)
        opt = default_options()
        for k, v in options.items():
            setattr(opt, k, v)
        self.ptr = C.c_void_p()
        rc = self.L.uvaia_align_open(C.byref(self.ptr), ref, len(ref), device, C.byref(opt))
        if rc:
            raise AlignError(rc, (self.L.uvaia_align_last_error(None) or b"").decode())
        self.n = 0

    def _chk(self, rc):
        if rc:
            raise AlignError(rc, (self.L.uvaia_align_last_error(self.ptr) or b"").decode())

    def close(self):
        if self.ptr:
            self.L.uvaia_align_close(self.ptr)
            self.ptr = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load(self, seqs):
        """seqs: list of bytes; they stay resident until the next load"""
        n = len(seqs)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        blob = b"".join(seqs)
        self._chk(self.L.uvaia_align_load_block(self.ptr, blob, off.ctypes.data_as(C.POINTER(C.c_int64)), n))
        self.n = n

    def load_device(self, d_bytes, offsets):
        """the pool from device memory: d_bytes a device pointer (an int), offsets n + 1 byte offsets from it (uvaia_align_load_device)"""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(off) - 1
        self.n = 0
        self._chk(self.L.uvaia_align_load_device(self.ptr, C.c_void_p(d_bytes), off.ctypes.data_as(C.POINTER(C.c_int64)), n))
        self.n = n

    def run(self):
        self._chk(self.L.uvaia_align_run(self.ptr))

    def fetch(self):
        rows = np.zeros((self.n, self.ref_len + 1), dtype=np.uint8)
        score = np.zeros(self.n, dtype=np.int32)
        self._chk(self.L.uvaia_align_fetch(self.ptr, rows.ctypes.data, score.ctypes.data_as(C.POINTER(C.c_int))))
        return score, rows[:, :self.ref_len]

    def device_rows(self):
        """(device pointer, pitch, n, device) of the rows of the last completed run: they stay where the kernel left them, valid until the
        next load or close, and go to capi.Engine.rows_census / db_append_device / rows_exceptions as they are"""
        ptr, pitch, n, dev = C.c_void_p(), C.c_size_t(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.uvaia_align_device_rows(self.ptr, C.byref(ptr), C.byref(pitch), C.byref(n), C.byref(dev)))
        return ptr.value or 0, pitch.value, n.value, dev.value

    def align(self, seqs):
        """(scores [n], aligned rows [n, ref_len]) through uvaia_align_batch, the reference-shaped call"""
        n = len(seqs)
        arr = (C.c_char_p * n)(*seqs)
        lens = (C.c_int * n)(*[len(s) for s in seqs])
        rows = np.zeros((n, self.ref_len + 1), dtype=np.uint8)
        score = np.zeros(n, dtype=np.int32)
        self._chk(self.L.uvaia_align_batch(self.ptr, arr, lens, n, rows.ctypes.data, score.ctypes.data_as(C.POINTER(C.c_int))))
        self.n = n
        return score, rows[:, :self.ref_len]

    def set_insertions(self, on, capacity=0):
        """keep the insertion runs of the following runs (uvaia_align_set_insertions); capacity: records a kernel launch has room for,
        0 = the library's choice (a launch that fills it runs the queries concerned again: nothing is lost)"""
        self._chk(self.L.uvaia_align_set_insertions(self.ptr, 1 if on else 0, capacity))

    def insertions(self):
        """the insertion runs of the last completed run as a list of (query, ref_pos, seq_pos, bases), sorted by (query, ref_pos)"""
        n_rec, n_bases = C.c_longlong(0), C.c_longlong(0)
        self._chk(self.L.uvaia_align_insertion_counts(self.ptr, C.byref(n_rec), C.byref(n_bases)))
        rec = (Insertion * max(n_rec.value, 1))()
        bases = C.create_string_buffer(max(n_bases.value, 1))
        self._chk(self.L.uvaia_align_fetch_insertions(self.ptr, C.cast(rec, C.c_void_p), C.cast(bases, C.c_void_p)))
        out, at, raw = [], 0, bases.raw
        for r in rec[:n_rec.value]:
            out.append((r.query, r.ref_pos, r.seq_pos, raw[at:at + r.length]))
            at += r.length
        return out

    def set_variants(self, on):
        """derive substitutions, deletions and per-row counts from the rows of the following runs (uvaia_align_set_variants)"""
        self._chk(self.L.uvaia_align_set_variants(self.ptr, 1 if on else 0))

    def variants(self):
        """(records, qc) of the last completed run with the option on, or of variants_of, whichever came last: numpy structured arrays of
        VARIANT_DTYPE (sorted by query, then ref_pos; kind is ord('S') or ord('D')) and QC_DTYPE (one entry per row)"""
        n_rec, n_rows = C.c_longlong(0), C.c_int(0)
        self._chk(self.L.uvaia_align_variant_counts(self.ptr, C.byref(n_rec), C.byref(n_rows)))
        rec = np.zeros(n_rec.value, dtype=VARIANT_DTYPE)
        qc = np.zeros(n_rows.value, dtype=QC_DTYPE)
        self._chk(self.L.uvaia_align_fetch_variants(self.ptr, rec.ctypes.data if rec.size else None, qc.ctypes.data if qc.size else None))
        return rec, qc

    def variants_of(self, rows, pitch=None):
        """records and counts of rows aligned elsewhere (uvaia_align_variants_of): rows is a 2-D uint8 array [n, >= ref_len], a list of
        bytes of ref_len characters each, or, with pitch, a flat buffer of rows pitch bytes apart.  Returns what variants() returns."""
        if pitch is None:
            if isinstance(rows, np.ndarray):
                arr = np.ascontiguousarray(rows, dtype=np.uint8)
                if arr.ndim != 2:
                    raise ValueError("rows: a 2-D array, or a flat buffer together with pitch")
            else:
                rows = list(rows)
                if any(len(r) != self.ref_len for r in rows):
                    raise ValueError("every row has ref_len = %d characters" % self.ref_len)
                arr = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), self.ref_len)
            n, pitch = arr.shape[0], (arr.shape[1] if arr.shape[0] else self.ref_len)
        else:
            arr = np.ascontiguousarray(np.frombuffer(rows, dtype=np.uint8) if not isinstance(rows, np.ndarray) else rows.reshape(-1), dtype=np.uint8)
            if pitch < 1 or (arr.size and arr.size < self.ref_len):
                raise ValueError("a flat buffer holds at least one row")
            n = 0 if not arr.size else (arr.size - self.ref_len) // pitch + 1
        self._chk(self.L.uvaia_align_variants_of(self.ptr, arr.ctypes.data if arr.size else None, pitch, n))
        return self.variants()

    def variants_ms(self, reset=False):
        """device time of the variant passes in ms since the aligner was opened or last reset; not part of stats()['kernel_ms']"""
        return float(self.L.uvaia_align_variants_ms(self.ptr, 1 if reset else 0))

    def stats(self):
        cells, nbytes, passes, ms = C.c_ulonglong(0), C.c_double(0), C.c_int(0), C.c_double(0)
        self._chk(self.L.uvaia_align_stats(self.ptr, C.byref(cells), C.byref(nbytes), C.byref(passes), C.byref(ms)))
        return {"cells": cells.value, "wavefront_bytes": nbytes.value, "passes": passes.value, "kernel_ms": ms.value}
