"""Helpers of the tests of rows in device memory on their way into the packed database: the host rules restated in Python (no GPU needed).

    count_non_n     quick_count_sequence_non_N (uvaia_amd/csrc/host/seq_query.c:105-115)
    exception_runs  the exception pass of uvdb_add_reference (uvaia_amd/csrc/host/uvdb.c)
"""
import numpy as np

EXCEPTIONS = b"-?XO."               # upper case only, as the writer takes them
RUN_CUT = 0xFFFFFF                  # a record keeps the length in 24 bits

_INVALID = np.zeros(256, dtype=bool)
for _c in b"NnXxOo-?.":
    _INVALID[_c] = True


def count_non_n(row):
    return int(len(row) - _INVALID[np.frombuffer(bytes(row), dtype=np.uint8)].sum())


def exception_runs(row, cut=RUN_CUT):
    """[(pos, len << 8 | char)]: a run is a maximal stretch of one of the exception characters; it is cut where the character changes and
    at a length of `cut`"""
    out, s, n = [], 0, len(row)
    while s < n:
        ch = row[s]
        if ch in EXCEPTIONS:
            e = s + 1
            while e < n and row[e] == ch and e - s < cut:
                e += 1
            out.append((s, ((e - s) << 8) | ch))
            s = e
        else:
            s += 1
    return out


def random_rows(n, nchar, seed, special=True):
    """text rows with every kind of site: ACGT, IUPAC codes in both cases, N runs, runs of every exception character (next to each other,
    at site 0, at the last site), lower-case x and o; with special, row 0 is all '-', row 1 all ACGT, row 2 one run with an N inside"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTacgtMRWSYKVHDBmrwsykvhdbNnxo", dtype=np.uint8)
    rows = []
    for i in range(n):
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar)
        pos = rng.choice(nchar, size=max(1, nchar // 8), replace=False)
        s[pos] = rng.choice(alphabet, size=len(pos))
        for ch in b"N-?.XO-":
            for _ in range(3):
                a = int(rng.integers(0, nchar))
                s[a:a + int(rng.integers(1, 90))] = ch
        if i % 3 == 0:
            s[:int(rng.integers(1, 40))] = ord("-")
            s[nchar - int(rng.integers(1, 40)):] = ord("?")
        if i % 5 == 1:
            a = int(rng.integers(0, max(1, nchar - 40)))
            s[a:a + 10] = ord("-"); s[a + 10:a + 20] = ord("."); s[a + 20:a + 21] = ord("N"); s[a + 21:a + 30] = ord("-")
        rows.append(s.tobytes())
    if special and n >= 3:
        rows[0] = b"-" * nchar
        rows[1] = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nchar))
        rows[2] = b"-" * (nchar // 2) + b"N" + b"-" * (nchar - nchar // 2 - 1)
    return rows
