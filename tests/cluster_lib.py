"""What the reference's `uvaiaclust` computes, for the tests: the C restatement (tests/cluster_restatement.c, built here into a
temporary directory), a second restatement in Python that transcribes the reference's loops with their shared score buffer, and
the text of the two output files."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def restatement():
    out = os.path.join(tempfile.mkdtemp(prefix="cluster_rs_"), "libcluster_rs.so")
    subprocess.check_call(["cc", "-O2", "-fopenmp", "-shared", "-fPIC", "-o", out, os.path.join(HERE, "cluster_restatement.c")])
    L = C.CDLL(out)
    pl = C.POINTER(C.c_int64)
    L.rs_cluster.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), pl, pl, pl, C.POINTER(C.c_int)]
    L.rs_cluster.restype = C.c_int
    L.rs_reference.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    L.rs_reference.restype = None
    L.rs_threads.restype = C.c_int
    return L


def rs_cluster(reference, seqs, queues, dist, trim=0, n_score=1, n_queues=None):
    """C restatement: [(medoid, [members])], scores [k, n_score + 2]"""
    L = restatement()
    n, nchar = len(seqs), len(reference)
    n_queues = n_queues or (int(max(queues)) + 1 if n else 1)
    blob = b"".join(seqs)
    q = np.ascontiguousarray(queues, dtype=np.int32)
    medoid, offsets, members = np.zeros(max(n, 1), np.int64), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.int64)
    scores = np.zeros((max(n, 1), n_score + 2), np.int32)
    pl = C.POINTER(C.c_int64)
    k = L.rs_cluster(reference, nchar, dist, trim, n_score, n_queues, n, blob, q.ctypes.data_as(C.POINTER(C.c_int)), medoid.ctypes.data_as(pl),
                     offsets.ctypes.data_as(pl), members.ctypes.data_as(pl), scores.ctypes.data_as(C.POINTER(C.c_int)))
    m, off, mem = medoid[:k].tolist(), offsets[:k + 1].tolist(), members.tolist()
    return [(m[i], mem[off[i]:off[i + 1]]) for i in range(k)], scores[:k]


def rs_reference(seqs):
    """read_reference_sequence over these records (the caller picks them: the first of -r, or up to 1024 of the first file)"""
    nchar = len(seqs[0])
    out = C.create_string_buffer(nchar)
    restatement().rs_reference(b"".join(seqs), len(seqs), nchar, out)
    return out.raw[:nchar]


def round_robin(file_sizes, n_queues):
    return [k % n_queues for n in file_sizes for k in range(n)]


def clamp(nchar, dist, trim, n_score):
    dist, n_score, trim = max(dist, 0), max(n_score, 0), max(trim, 0)
    if trim > nchar / 2.1:
        trim = int(nchar / 2.1)
    if dist > nchar // 10:
        dist = nchar // 10
    return dist, trim, n_score


def csv_text(clusters, names):
    return "".join(",".join([names[m]] + [names[x] for x in mem]) + "\n" for m, mem in clusters)


def aln_records(clusters, names, seqs):
    return [(names[m], seqs[m].upper()) for m, _ in clusters]


def families(n, n_fam, seed):
    """n sequences of n_fam families: a row of the clean synthetic preset plus 0-4 random substitutions and, for 30 %, an N run"""
    from uvaia_amd import hostlib
    g = hostlib.Synth(seed=seed, preset=1)
    base, _ = g.generate(0, n_fam)
    rng = np.random.default_rng(seed)
    L = base.shape[1]
    rows = base[rng.integers(0, n_fam, n)].copy()
    for i in range(n):
        k = rng.integers(0, 5)
        rows[i, rng.integers(0, L, k)] = rng.choice(np.frombuffer(b"ACGT", np.uint8), k)
        if rng.random() < 0.3:
            a = int(rng.integers(0, L - 300))
            rows[i, a:a + int(rng.integers(1, 300))] = ord("N")
    return [rows[i].tobytes() for i in range(n)]


# ----------------------------------------------------------------------------------------------------------- Python transcription
class _Fs:
    def __init__(self, n_score):
        self.nn, self.name, self.seq, self.score = [], None, None, [0] * (n_score + 2)


def py_cluster(reference, seqs, queues, dist, trim, n_score, n_queues):
    """src/cluster.c:157-237 with src/fastaseq.c's loops, one score buffer per call as there (list indices for pointers)"""
    nchar = len(reference)
    valid = lambda a, b: a != 0 and b != 0                          # is_site_pair_valid with the tables left uninitialised
    pad = bytes(trim + 16)

    def at(s, i):
        return s[i] if i < len(s) else 0

    class Cl:
        pass

    cq = []
    for _ in range(n_queues):
        k = Cl()
        k.fs, k.idx, k.n_idx = [], [0] * nchar, nchar
        cq.append(k)

    def add_seq_to_cluster(clust, idx, seq, name, score):
        if idx >= len(clust.fs):
            f = _Fs(n_score)
            clust.fs.append(f)
            f.seq, f.name, f.score = seq, name, list(score[:n_score + 2])
            return
        if score[n_score + 1] > clust.fs[idx].score[n_score + 1]:
            f = clust.fs[idx]
            f.seq = seq
            f.nn.append(f.name)
            f.name, f.score = name, list(score[:n_score + 2])
            return
        clust.fs[idx].nn.append(name)

    def check(clust, seq, name):
        score = [0] * (n_score + 2)
        score[n_score + 1] = sum(1 for c in seq[:nchar] if c != 0)
        s1, s2, ns = trim, trim, nchar - 2 * trim
        score[0] = 0
        for i in range(1, n_score + 1):
            score[i] = -1
        for i in range(ns):
            a, b = seq[s1 + i], reference[s2 + i]
            if not valid(a, b):
                continue
            score[0] += 1
            if a == b:
                score[0] -= 1
            else:
                clust.idx[i] += 1
            if n_score and score[0] and score[0] <= n_score and score[score[0]] < 0:
                score[score[0]] = i
        i = 0
        while i < len(clust.fs):
            f = clust.fs[i]
            if abs(score[0] - f.score[0]) <= dist:
                minloc = (min(score[1], f.score[1]) - 1) if n_score else 0
                minloc = max(minloc, 0)
                score[0] = 0
                j = 0
                while j < ns and score[0] < dist + 1:
                    a, b = at(seq, trim + minloc + j), at(f.seq, trim + minloc + j)
                    j += 1
                    if not valid(a, b):
                        continue
                    score[0] += 1
                    if a == b:
                        score[0] -= 1
                if score[0] <= dist:
                    add_seq_to_cluster(clust, i, seq, name, score)
                    return
            i += 1
        add_seq_to_cluster(clust, i, seq, name, score)

    for o, (s, q) in enumerate(zip(seqs, queues)):
        check(cq[q], s.upper() + pad, o)

    # generate_idx_from_cluster_list (src/fastaseq.c:127-138)
    tot = [sum(k.idx[i] for k in cq) for i in range(nchar)]
    idx = [i for i in range(nchar) if tot[i] > 0]

    def key(f):
        return tuple(-x for x in f.score)

    def merge(c1, c2):
        if not c2.fs:
            return
        c1.fs.sort(key=key)
        c2.fs.sort(key=key)
        if not c1.fs:
            c1.fs, c2.fs = c2.fs, []
            return
        n1 = len(c1.fs)
        for f2 in c2.fs:
            c2s, hit = f2.score[0], None
            for i in range(n1):
                f1 = c1.fs[i]
                if abs(c2s - f1.score[0]) > dist:
                    continue
                d = 0
                for x in idx:
                    if d >= dist + 1:
                        break
                    if f1.seq[trim + x] != f2.seq[trim + x]:
                        d += 1
                if d <= dist:
                    hit = f1
                    break
            if hit is not None:
                hit.nn.append(f2.name)
                hit.nn.extend(f2.nn)
            else:
                c1.fs.append(f2)
        c2.fs = []

    c = n_queues
    while c > 1:
        for j in range(c // 2):
            merge(cq[j], cq[j + c // 2 + c % 2])
        c = c // 2 + c % 2
    final = sorted(cq[0].fs, key=lambda f: (-len(f.nn),) + key(f))
    return [(f.name, list(f.nn)) for f in final], np.array([f.score for f in final], dtype=np.int32).reshape(len(final), n_score + 2)
