"""ctypes binding of include/uvaia_cluster.h (tests and tools reach the clustering of `uvaiaclust` through it)."""
import ctypes as C

import numpy as np

from . import capi

# every symbol include/uvaia_cluster.h declares (tests check the library exports all of them)
SYMBOLS = [
    "uvaia_clust_open", "uvaia_clust_close", "uvaia_clust_last_error", "uvaia_clust_push", "uvaia_clust_finish", "uvaia_clust_result",
    "uvaia_clust_stats", "uvaia_clust_push_packed", "uvaia_clust_rows", "uvaia_clust_device_rows", "uvaia_clust_unpack_ms",
    "uvaia_clust_keep_medoids", "uvaia_clust_gather_device", "uvaia_clust_memory", "uvaia_clust_push_device", "uvaia_clust_push_device_ms",
]


class ClusterError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("uvaia_clust error %d: %s" % (code, msg))
        self.code = code


_ready = False


def _lib():
    global _ready
    L = capi.load_library()
    if not _ready:
        vp, pi, pl = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)
        L.uvaia_clust_open.argtypes = [C.POINTER(vp), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.uvaia_clust_close.argtypes = [vp]
        L.uvaia_clust_close.restype = None
        L.uvaia_clust_last_error.argtypes = [vp]
        L.uvaia_clust_last_error.restype = C.c_char_p
        L.uvaia_clust_push.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), pi]
        L.uvaia_clust_finish.argtypes = [vp]
        L.uvaia_clust_result.argtypes = [vp, pi, pl, pl, pl, pi]
        L.uvaia_clust_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), pl]
        L.uvaia_clust_push_packed.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_uint64), vp, pi]
        L.uvaia_clust_rows.argtypes = [vp, pl, C.c_int, vp, C.c_size_t]
        L.uvaia_clust_device_rows.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.uvaia_clust_unpack_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.uvaia_clust_keep_medoids.argtypes = [vp, C.c_int]
        L.uvaia_clust_gather_device.argtypes = [vp, pl, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.uvaia_clust_memory.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.uvaia_clust_push_device.argtypes = [vp, C.c_int, vp, C.c_size_t, pi, pi]
        L.uvaia_clust_push_device_ms.argtypes = [vp, C.POINTER(C.c_double)]
        _ready = True
    return L


class Result:
    """The clusters in their final order: medoid push ordinals, member lists (without the medoid) and stored score vectors."""

    def __init__(self, medoid, offsets, members, scores):
        self.medoid, self.offsets, self.members, self.scores = medoid, offsets, members, scores

    def clusters(self):
        """[(medoid, [members...]), ...] as Python ints"""
        m, off, mem = self.medoid.tolist(), self.offsets.tolist(), self.members.tolist()
        return [(m[k], mem[off[k]:off[k + 1]]) for k in range(len(m))]


class Clusterer:
    """One clustering on one GPU (new_cqueue, src/cluster.c:280-300): parameters already clamped by the caller."""

    def __init__(self, reference, dist=1, trim=0, n_score=1, n_queues=1, device=0):
        self.L = _lib()
        self.n_score = n_score
        self.ptr = C.c_void_p()
        rc = self.L.uvaia_clust_open(C.byref(self.ptr), device, reference, len(reference), dist, trim, n_score, n_queues)
        if rc:
            raise ClusterError(rc, (self.L.uvaia_clust_last_error(None) or b"").decode())
        self.pushed = 0
        self.nchar = len(reference)

    def _chk(self, rc):
        if rc:
            raise ClusterError(rc, (self.L.uvaia_clust_last_error(self.ptr) or b"").decode())

    def close(self):
        if self.ptr:
            self.L.uvaia_clust_close(self.ptr)
            self.ptr = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, seqs, queues):
        """seqs: list of bytes of the reference's length; queues: the queue of each"""
        n = len(seqs)
        if not n:
            return
        arr = (C.c_char_p * n)(*seqs)
        q = np.ascontiguousarray(queues, dtype=np.int32)
        self._chk(self.L.uvaia_clust_push(self.ptr, n, arr, q.ctypes.data_as(C.POINTER(C.c_int))))
        self.pushed += n

    def push_packed(self, planes, n, exc_offsets, exc, queues):
        """n sequences as ceil(n / 64) whole tiles of the packed interchange form (planes: uint8 array) with their exception runs:
        exc_offsets (n + 1 record positions into exc, or None for no records) and exc (uint32 [records, 2]: pos, len << 8 | char)"""
        if not n:
            return
        planes = np.ascontiguousarray(planes, dtype=np.uint8).reshape(-1)
        tile = ((self.nchar + 31) // 32 + 3) // 4 * 4096
        if planes.size < (n + 63) // 64 * tile:
            raise ValueError("%d sequences need %d tiles of %d bytes" % (n, (n + 63) // 64, tile))
        q = np.ascontiguousarray(queues, dtype=np.int32)
        if len(q) != n:
            raise ValueError("one queue per sequence")
        off = rec = None
        if exc_offsets is not None:
            off = np.ascontiguousarray(exc_offsets, dtype=np.uint64)
            rec = np.ascontiguousarray(exc, dtype=np.uint32).reshape(-1, 2)
            if len(off) != n + 1 or (n and int(off[-1]) > len(rec)):
                raise ValueError("exc_offsets: n + 1 record positions inside exc")
        self._chk(self.L.uvaia_clust_push_packed(self.ptr, n, planes.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_uint64)) if off is not None else None,
                                                 rec.ctypes.data if rec is not None and len(rec) else None, q.ctypes.data_as(C.POINTER(C.c_int))))
        self.pushed += n

    def push_device(self, d_rows, pitch, queues, row_index=None):
        """sequences that are text rows in device memory: row row_index[i] (None: row i) of the block at device address d_rows, `pitch`
        bytes apart; one queue per pushed sequence"""
        q = np.ascontiguousarray(queues, dtype=np.int32)
        n = len(q)
        ri = None
        if row_index is not None:
            ri = np.ascontiguousarray(row_index, dtype=np.int32)
            if len(ri) != n:
                raise ValueError("one queue per selected row")
        if not n:
            return
        self._chk(self.L.uvaia_clust_push_device(self.ptr, n, d_rows, int(pitch), ri.ctypes.data_as(C.POINTER(C.c_int)) if ri is not None else None,
                                                 q.ctypes.data_as(C.POINTER(C.c_int))))
        self.pushed += n

    def push_device_ms(self):
        a = C.c_double(0)
        self._chk(self.L.uvaia_clust_push_device_ms(self.ptr, C.byref(a)))
        return a.value

    def rows(self, ordinals):
        """upper-case text of pushed sequences (push ordinals, any order, repeats allowed) as a list of bytes"""
        o = np.ascontiguousarray(ordinals, dtype=np.int64)
        buf = np.zeros((max(len(o), 1), self.nchar), dtype=np.uint8)
        self._chk(self.L.uvaia_clust_rows(self.ptr, o.ctypes.data_as(C.POINTER(C.c_int64)), len(o), buf.ctypes.data, self.nchar))
        return [buf[k].tobytes() for k in range(len(o))]

    def keep_medoids(self, slab_rows=0):
        """before the first push: keep the rows of the sequences that found a cluster only, in slabs of slab_rows rows (0: the default)"""
        self._chk(self.L.uvaia_clust_keep_medoids(self.ptr, slab_rows))

    def device_rows(self):
        """(device address of the row store, pitch): sequence o at address + o * pitch"""
        p, pitch = C.c_void_p(), C.c_size_t(0)
        self._chk(self.L.uvaia_clust_device_rows(self.ptr, C.byref(p), C.byref(pitch)))
        return p.value, pitch.value

    def gather_device(self, ordinals):
        """(device address, pitch) of these sequences gathered contiguously in device memory; valid until the next call on the context"""
        o = np.ascontiguousarray(ordinals, dtype=np.int64)
        p, pitch = C.c_void_p(), C.c_size_t(0)
        self._chk(self.L.uvaia_clust_gather_device(self.ptr, o.ctypes.data_as(C.POINTER(C.c_int64)), len(o), C.byref(p), C.byref(pitch)))
        return p.value, pitch.value

    def memory(self):
        a, b, f = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._chk(self.L.uvaia_clust_memory(self.ptr, C.byref(a), C.byref(b), C.byref(f)))
        return {"row_bytes": a.value, "peak_row_bytes": b.value, "free_bytes": f.value}

    def unpack_ms(self):
        a, b = C.c_double(0), C.c_double(0)
        self._chk(self.L.uvaia_clust_unpack_ms(self.ptr, C.byref(a), C.byref(b)))
        return {"decode_ms": a.value, "overlay_ms": b.value}

    def finish(self):
        self._chk(self.L.uvaia_clust_finish(self.ptr))

    def result(self):
        nc = C.c_int(0)
        self._chk(self.L.uvaia_clust_result(self.ptr, C.byref(nc), None, None, None, None))
        k = nc.value
        medoid = np.zeros(k, dtype=np.int64)
        offsets = np.zeros(k + 1, dtype=np.int64)
        members = np.zeros(max(self.pushed - k, 1), dtype=np.int64)
        scores = np.zeros((max(k, 1), self.n_score + 2), dtype=np.int32)
        pl = C.POINTER(C.c_int64)
        self._chk(self.L.uvaia_clust_result(self.ptr, C.byref(nc), medoid.ctypes.data_as(pl), offsets.ctypes.data_as(pl), members.ctypes.data_as(pl),
                                            scores.ctypes.data_as(C.POINTER(C.c_int))))
        return Result(medoid, offsets, members[:self.pushed - k], scores[:k])

    def stats(self):
        a, b, c, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int64(0)
        self._chk(self.L.uvaia_clust_stats(self.ptr, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"prep_ms": a.value, "queue_ms": b.value, "merge_ms": c.value, "pushed": n.value}


def exception_runs(seqs, cut=0xFFFFFF):
    """(exc_offsets uint64 [n + 1], exc uint32 [records, 2]) of these texts, by the rule of a packed database file: a maximal stretch
    of one of - ? X O . is a record (pos, len << 8 | char), cut every `cut` sites"""
    off, rec = [0], []
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8)
        hit = np.isin(a, np.frombuffer(b"-?XO.", dtype=np.uint8))
        if hit.any():
            start = np.flatnonzero(hit & np.concatenate(([True], (a[1:] != a[:-1]) | ~hit[:-1])))
            end = np.flatnonzero(hit & np.concatenate(((a[1:] != a[:-1]) | ~hit[1:], [True]))) + 1
            for b, e in zip(start.tolist(), end.tolist()):
                for p in range(b, e, cut):
                    rec.append((p, (min(cut, e - p) << 8) | int(a[b])))
        off.append(len(rec))
    return np.array(off, dtype=np.uint64), np.array(rec, dtype=np.uint32).reshape(-1, 2)


def queues_round_robin(file_sizes, n_queues):
    """src/cluster.c:164-181: within each input file sequence k goes to queue k mod Q; the next file starts again at queue 0"""
    return np.concatenate([np.arange(n, dtype=np.int32) % n_queues for n in file_sizes]) if file_sizes else np.zeros(0, dtype=np.int32)


def clamp_parameters(nchar, dist, trim, n_score):
    """src/cluster.c:131-132 and new_cqueue (src/cluster.c:287-289)"""
    dist = max(dist, 0)
    n_score = max(n_score, 0)
    trim = max(trim, 0)
    if trim > nchar / 2.1:
        trim = int(nchar / 2.1)
    if dist > nchar // 10:
        dist = nchar // 10
    return dist, trim, n_score
