"""What the tests of `uvaialign --device-parse` share: fasta_count_acgt_host and biomcmc_count_sequence_acgt of the host library through
ctypes, the Python restatement of the count, and the texts at the edges of fasta_sequences_kernel."""
import ctypes as C

import numpy as np

import fasta_lib as FL
from uvaia_amd import capi, hostlib

ACGT = frozenset(b"ACGTacgt")
INVALID = b"NnXxOo-?."                                                  # the "N etc." set of both counting functions
EDGE_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 9000)   # around a piece of 16 bytes, around a tile of the stage, beyond two tiles
GUARD = 64


def _lib():
    L = hostlib.load_library()
    if not getattr(L, "_align_parse_ready", False):
        L.fasta_count_acgt_host.restype = C.c_int
        L.fasta_count_acgt_host.argtypes = [C.c_void_p, C.c_void_p]
        L.biomcmc_count_sequence_acgt.restype = None
        L.biomcmc_count_sequence_acgt.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]
        L._align_parse_ready = True
    return L


def count_acgt_host(text, rec):
    """fasta_count_acgt_host per record of a table"""
    L = _lib()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    out = []
    for r in rec:
        one = np.array([r], dtype=capi.FASTA_RECORD_DTYPE)
        out.append(L.fasta_count_acgt_host(buf.ctypes.data, one.ctypes.data))
    return np.array(out, dtype=np.int32)


def count_sequence_acgt(seq):
    """biomcmc_count_sequence_acgt: the three fractions"""
    res = (C.c_double * 3)()
    _lib().biomcmc_count_sequence_acgt(bytes(seq), len(seq), res)
    return tuple(res)


def count_acgt_python(seq):
    return sum(1 for c in seq if c in ACGT)


def alphabet_corpus():
    """[(label, text)]: every character of the invalid set, in both cases where it has two, IUPAC codes, lower case, wrapped and CRLF bodies"""
    out = []
    body = b"ACGTacgt" + INVALID + b"RYKMSWBDHVrykmswbdhv" + b"ACGT" * 9 + INVALID * 3 + b"acgtu*JZ"
    out.append(("one_line", FL.fasta([b"a"], [body])))
    out.append(("wrap7", FL.fasta([b"a", b"b"], [body, body[::-1]], wrap=7)))
    out.append(("crlf_wrap60", FL.fasta([b"a", b"b"], [body * 5, body.lower() * 3], wrap=60, eol=b"\r\n")))
    for ch in INVALID:
        out.append(("only_%d" % ch, FL.fasta([b"x", b"y"], [bytes([ch]) * 37, b"AC" + bytes([ch]) + b"gt"], wrap=10)))
    out.append(("no_acgt", FL.fasta([b"n"], [b"NNNNRYRY----"])))
    return out


def _shape(i, name, s):
    """record i of an edge text: the body on one line, wrapped at 60 and at 70, with CRLF, with blank lines inside, in lower case"""
    how = i % 6
    if how == 0:
        return FL.fasta([name], [s])
    if how == 1:
        return FL.fasta([name], [s], wrap=60)
    if how == 2:
        return FL.fasta([name], [s], wrap=70)
    if how == 3:
        return FL.fasta([name], [s], wrap=60, eol=b"\r\n")
    if how == 4:
        k = len(s) // 2
        return b">" + name + b"\n" + s[:k] + b"\n\n \t\n" + s[k:] + b"\n\r\n"
    return FL.fasta([name], [s.lower()], wrap=70)


def edge_corpus():
    """one text whose cleaned lengths are those of EDGE_LENGTHS (some twice and more), in an order that puts a sequence at every residue
    modulo 16 of the buffer fasta_sequences fills: sixteen lengths that are 1 modulo 16 first, then the rest.  (text, lengths)"""
    lengths = [1, 17, 33, 4097] * 4 + [n for n in EDGE_LENGTHS if n % 16 != 1]
    text = b""
    for i, n in enumerate(lengths):
        text += _shape(i + i // 6, b"e%d len %d" % (i, n), FL.sequences(1, n, 1000 + i)[0])      # (i + i // 6: a length meets more than one shape)
    return text, lengths


def chunk_corpus(chunk):
    """a body that spans two pass-1 chunks, one that spans three, and a header line that crosses a chunk boundary"""
    a, b, c = FL.sequences(3, 2 * chunk + 100, 77)
    text = b">two\n" + a[:chunk + 50] + b"\n"                          # from byte 5 into the second chunk
    text += b">three wrapped\n" + b"".join(b[i:i + 60] + b"\n" for i in range(0, len(b), 60))
    lead = (-len(text) - 10) % chunk                                     # the next header line begins 10 bytes in front of a boundary
    lead += chunk if lead < 7 else 0
    text += b">pad\n" + c[:lead - 6] + b"\n"
    at = len(text)
    text += b">a name that lies across the boundary\n" + c[:chunk + 1].lower() + b"\n>last\nACGTN\n"
    assert at % chunk == chunk - 10 and text[at:at + 1] == b">"
    return text
