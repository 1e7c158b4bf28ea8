"""FASTA texts for the tests of the device parser (`uvaiapack --device-parse`) and the plain C restatement of its first pass,
fasta_scan_host of uvaia_amd/csrc/host/fasta_blocks.c, through ctypes.

Every text of corpus() is regular: readfasta_next (uvaia_amd/csrc/host/seq_query.c) reads it without guessing, so the line reader, the C
restatement and the device must agree on its names and cleaned sequences."""
import ctypes as C

import numpy as np

from uvaia_amd import capi, hostlib

BAD_NUL, BAD_TEXT, BAD_EMPTY = 1, 2, 3
PLACES = (15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)      # and the scan's chunk size - 1, + 0, + 1


class FastaBad(Exception):
    def __init__(self, kind, off):
        super().__init__("kind %d at offset %d" % (kind, off))
        self.kind, self.off = kind, off


def _lib():
    L = hostlib.load_library()
    if not getattr(L, "_fasta_ready", False):
        L.fasta_scan_host.restype = C.c_int
        L.fasta_scan_host.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        L.fasta_clean_host.restype = C.c_size_t
        L.fasta_clean_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.fasta_blocks_normalise_host.restype = C.c_int
        L.fasta_blocks_normalise_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t]
        L._fasta_ready = True
    return L


def scan_host(text, final=True, max_records=4096):
    """fasta_scan_host: (table as a structured array, consumed); FastaBad on irregular input"""
    L = _lib()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    rec = np.zeros(max_records, dtype=capi.FASTA_RECORD_DTYPE)
    n, cons, kind, off = C.c_int(0), C.c_size_t(0), C.c_int(0), C.c_size_t(0)
    rc = L.fasta_scan_host(buf.ctypes.data if buf.size else None, buf.size, int(bool(final)), max_records, rec.ctypes.data, C.byref(n), C.byref(cons), C.byref(kind), C.byref(off))
    if rc:
        raise FastaBad(kind.value, off.value)
    return rec[:n.value].copy(), cons.value


def clean_host(text, rec):
    """the cleaned sequences of the records of a table, by fasta_clean_host"""
    L = _lib()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    out = []
    for r in rec:
        one = np.array([r], dtype=capi.FASTA_RECORD_DTYPE)
        seq = np.zeros(int(r["seq_len"]) + 1, dtype=np.uint8)
        n = L.fasta_clean_host(buf.ctypes.data, one.ctypes.data, seq.ctypes.data)
        assert n == r["seq_len"]
        out.append(seq[:n].tobytes())
    return out


def names_of(text, rec):
    return [bytes(text[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])]) for r in rec]


def normalise_host(path, block_bytes, out_path, max_records=4096):
    """the file through the block reader and fasta_scan_host, as ">name\\nSEQUENCE\\n" per record; the message where it is refused"""
    err = C.create_string_buffer(1024)
    rc = _lib().fasta_blocks_normalise_host(str(path).encode(), block_bytes, max_records, str(out_path).encode(), err, len(err))
    return None if rc == 0 else err.value.decode()


def read_with_line_reader(path):
    """[(name, sequence)] as readfasta_next gives them"""
    L = hostlib.load_library()
    r = L.new_readfasta(str(path).encode())
    out = []
    try:
        while L.readfasta_next(r) >= 0:
            c = r.contents
            out.append((c.name, C.string_at(c.seq, c.seqlength)))
            if not c.seqfile:
                break
    finally:
        L.del_readfasta(r)
    return out


def normal_form(pairs):
    return b"".join(b">" + n + b"\n" + s + b"\n" for n, s in pairs)


# ---------------------------------------------------------------------------------------------------------------- texts
def sequences(n, nchar, seed, lower=False):
    """n rows of nchar sites over the whole alphabet of a reference file, mostly ACGT"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT" * 12 + b"NRYKMSWBDHV-?XO.", dtype=np.uint8)
    rows = alpha[rng.integers(0, len(alpha), size=(n, nchar))]
    out = [r.tobytes() for r in rows]
    return [s.lower() if lower else s for s in out]


def fasta(names, seqs, wrap=None, eol=b"\n", last_eol=True):
    out = []
    for nm, s in zip(names, seqs):
        out.append(b">" + nm + eol)
        w = wrap or max(len(s), 1)
        for a in range(0, len(s), w):
            out.append(s[a:a + w] + eol)
    text = b"".join(out)
    return text if last_eol else text[:len(text) - len(eol)]


def _names(n, tag):
    return [("%s%d" % (tag, i)).encode() for i in range(n)]


SHAPE_NCHAR = 130


def size_corpus():
    """[(label, text)]: one line per sequence, rows of 29 to 29 903 sites, 1 to 130 records"""
    out = []
    for nchar, n in ((29, 130), (64, 65), (65, 64), (1000, 63), (29903, 1), (29903, 3)):
        out.append(("one_line_%dx%d" % (n, nchar), fasta(_names(n, "s%d_" % n), sequences(n, nchar, 100 + nchar + n))))
    return out


def shape_corpus(nchar=SHAPE_NCHAR):
    """[(label, text)]: the line shapes and header shapes, every record of nchar sites (one `uvaiapack` command takes them all)"""
    out = []
    s = sequences(9, nchar, 7)
    out.append(("wrap60", fasta(_names(9, "w"), s, wrap=60)))
    out.append(("wrap70_crlf", fasta(_names(9, "c r"), s, wrap=70, eol=b"\r\n")))
    out.append(("wrap1", fasta(_names(5, "o"), sequences(5, nchar, 8), wrap=1)))
    out.append(("no_last_newline", fasta(_names(4, "e"), sequences(4, nchar, 9), wrap=60, last_eol=False)))
    out.append(("crlf_no_last_newline", fasta(_names(3, "f"), sequences(3, nchar, 10), eol=b"\r\n")[:-1]))          # ends in '\r'
    mixed = [bytes(c + 32 if (i % 3 == 0 and 65 <= c <= 90) else c for i, c in enumerate(q)) for q in sequences(6, nchar, 11)]
    out.append(("mixed_case", fasta(_names(6, "m"), mixed, wrap=60)))
    out.append(("lower_case", fasta(_names(6, "l"), sequences(6, nchar, 12, lower=True))))
    # blank and white-space-only lines between and inside records, spaces and tabs inside sequence lines
    t = b"\n \t\n"
    for i, q in enumerate(sequences(4, nchar, 13)):
        t += b">b %d\n" % i + q[:10] + b" " + q[10:17] + b"\t\n\n \x0b\x0c\r\n" + q[17:30] + b"\n\t" + q[30:] + b" \n\n"
    out.append(("blank_lines_and_spaces", t))
    # names: empty, with spaces and further '>', a header line whose first byte is not '>'
    s = sequences(5, nchar, 14)
    t = b">\n" + s[0] + b"\n> \n" + s[1] + b"\n>a b>c >> d\n" + s[2] + b"\nxy>after text\n" + s[3] + b"\n \t>after blanks>\r\n" + s[4] + b"\n"
    out.append(("names", t))
    return out


def aligned_corpus():
    """[(label, text)]: every record of a text has the same length (what `uvaiapack` takes)"""
    return size_corpus() + shape_corpus()


def ragged_corpus(chunk):
    """[(label, text)]: regular texts whose records differ in length: bytes >= 0x80, and a '>' and a '\\n' at each place of PLACES and around
    the scan's chunk size, with the start of the line close by and far in front"""
    out = []
    out.append(("high_bytes", b">h\xc3\xa9\n" + bytes(range(0x80, 0x100)) + b"\nAC\xff\xfeGT\n>i\n\x80a\x01z{`@[\n"))
    tail = b">z y>w\nacgtn-\nNNAC\n"
    for p in PLACES + (chunk - 1, chunk, chunk + 1):
        a = sequences(1, p, p)[0]
        # '>' at p, its line begins at p - 1 (a header line "x>...")
        out.append(("gt_%d_near" % p, b">p\n" + a[:p - 5] + b"\n" + b"x>near %d\nACGTAC\n" % p + tail))
        # '>' at p, its line begins at 0 (p <= 17) or right behind a record of five bytes
        head = b"" if p <= 17 else b">a\nA\n"
        out.append(("gt_%d_far" % p, head + b"y" * (p - len(head)) + b">far %d\nACGTAC\n" % p + tail))
        # '\n' at p: the end of a sequence line of one byte, and of one that began behind the header
        out.append(("nl_%d_near" % p, b">n\n" + a[:p - 5] + b"\n" + a[p - 5:p - 4] + b"\n" + a[:7] + b"\n" + tail))
        out.append(("nl_%d_far" % p, b">n\n" + a[:p - 3] + b"\n" + a[:7] + b"\n" + tail))
    for label, t in out:
        if label.startswith("gt_"):
            p = int(label.split("_")[1])
            assert t[p:p + 1] == b">" and b">" not in t[t.rfind(b"\n", 0, p) + 1:p], label
        if label.startswith("nl_"):
            assert t[int(label.split("_")[1]):][:1] == b"\n", label
    return out


def corpus(chunk=4096):
    return aligned_corpus() + ragged_corpus(chunk)
