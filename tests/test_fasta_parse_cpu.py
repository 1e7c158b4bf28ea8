"""`uvaiapack --device-parse`, the part that needs no GPU: fasta_scan_host (the plain C restatement of the device parser's first pass) against
readfasta_next, the block reader of uvaia_amd/csrc/host/fasta_blocks.c at every block size, the exported symbols, the layout of the record
table, and what the command refuses while it reads its options."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import fasta_lib as FL
from uvaia_amd import capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIAPACK = os.path.join(ROOT, "bin", "uvaiapack")


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build_library()


def test_scan_host_agrees_with_the_line_reader_on_every_regular_text(tmp_path):
    for label, text in FL.corpus():
        p = tmp_path / (label + ".fa")
        p.write_bytes(text)
        want = FL.read_with_line_reader(p)
        rec, consumed = FL.scan_host(text, final=True)
        assert consumed == len(text), label
        assert not rec["flags"].any(), label
        got = list(zip(FL.names_of(text, rec), FL.clean_host(text, rec)))
        assert got == want, label
        L = hostlib.load_library()
        assert [int(r["non_n"]) for r in rec] == [L.quick_count_sequence_non_N(s, len(s)) for _, s in want], label


def test_scan_host_contract_at_the_cap_and_the_cut():
    text = FL.fasta([b"a", b"b b", b"c"], [b"ACGT", b"acgtn", b"AC-T"])
    # not final: the last record is not complete, consumed is where its header line begins
    rec, consumed = FL.scan_host(text, final=False)
    assert len(rec) == 2 and consumed == text.index(b">c")
    # a cut inside the next header line completes the record in front of it only once its '>' is there
    cut = text.index(b">c")
    assert len(FL.scan_host(text[:cut], final=False)[0]) == 1
    assert len(FL.scan_host(text[:cut + 1], final=False)[0]) == 2
    # the cap: consumed stops there and a second call goes on
    rec, consumed = FL.scan_host(text, final=True, max_records=2)
    assert len(rec) == 2 and consumed == text.index(b">c")
    rec, c2 = FL.scan_host(text[consumed:], final=True, max_records=2)
    assert len(rec) == 1 and c2 == len(text) - consumed and FL.clean_host(text[consumed:], rec) == [b"AC-T"]
    # blank text is consumed whole; a record that does not end leaves everything
    assert FL.scan_host(b"\n \n", final=False) [1] == 3
    rec, consumed = FL.scan_host(b">only\nACGT", final=False)
    assert len(rec) == 0 and consumed == 0


def test_scan_host_reports_irregular_input_by_kind_and_offset():
    for text, kind, off in ((b">a\nAC\x00GT\n>b\nAC\n", FL.BAD_NUL, 5), (b"\x00>a\nAC\n", FL.BAD_NUL, 0), (b">a\x00\nAC\n", FL.BAD_NUL, 2),
                            (b"\n ACGT\n>a\nAC\n", FL.BAD_TEXT, 2), (b">a\nAC\n>b\n>c\nAC\n", FL.BAD_EMPTY, 6), (b">a\nAC\n>b\n \n", FL.BAD_EMPTY, 6),
                            (b">a\nAC\n>b", FL.BAD_EMPTY, 6)):
        with pytest.raises(FL.FastaBad) as e:
            FL.scan_host(text, final=True)
        assert (e.value.kind, e.value.off) == (kind, off), text
    # an empty record that is not complete yet is no finding
    assert len(FL.scan_host(b">a\nAC\n>b\n", final=False)[0]) == 1


def _through_blocks(tmp_path, text, block):
    src, out = tmp_path / "in.fa", tmp_path / "out.fa"
    src.write_bytes(text)
    err = FL.normalise_host(src, block, out)
    return err, (out.read_bytes() if err is None else None)


def test_block_reader_at_every_block_size(tmp_path):
    names, seqs = [b"first", b"second one", b""], [b"ACGTNNACGT" * 3, b"acgtacgtac" * 5 + b"GG", b"TTTT"]
    text = FL.fasta(names, seqs, wrap=10)
    want = FL.normal_form(zip(names, [s.upper() for s in seqs]))
    longest = max(len(FL.fasta([n], [s], wrap=10)) for n, s in zip(names, seqs))
    for block in range(longest + 1, len(text) + 1):
        err, got = _through_blocks(tmp_path, text, block)
        assert err is None and got == want, (block, err)
    # a block of the longest record's size cannot hold it together with the '>' that completes it: refused by name
    err, _ = _through_blocks(tmp_path, text, longest)
    assert err is not None and "second one" in err and "does not fit" in err


def test_block_reader_cuts(tmp_path):
    """the first block ends inside a header, after a header's newline, inside a sequence line, between '\\r' and '\\n', and between x and > of a
    header line x>name; the record in front of the cut is carried to the next block unless the '>' behind it was seen"""
    text = b">zero\nAC\n>one\r\nACGTACGTAC\r\nGGTTAACC\r\nx>two words\r\nacgtacgtacgtac\r\n>three\r\nAC\r\n"
    want = FL.normal_form([(b"zero", b"AC"), (b"one", b"ACGTACGTACGGTTAACC"), (b"two words", b"ACGTACGTACGTAC"), (b"three", b"AC")])
    cuts = {"inside a header": text.index(b"two") + 2, "after a header's newline": text.index(b"acgt"), "inside a sequence line": text.index(b"acgt") + 5,
            "between CR and LF": text.index(b"acgtacgtacgtac") + 15, "between x and >": text.index(b"x>two") + 1}
    assert text[cuts["between CR and LF"] - 1:][:2] == b"\r\n" and text[cuts["between x and >"] - 1:][:2] == b"x>"
    for what, cut in cuts.items():
        err, got = _through_blocks(tmp_path, text, cut)
        assert err is None and got == want, (what, err)
    # without a record in front, a block that ends between x and > holds no complete record: refused by name, nothing is guessed
    err, _ = _through_blocks(tmp_path, text[text.index(b">one"):], cuts["between x and >"] - text.index(b">one"))
    assert err is not None and "'one" in err and "does not fit" in err


def test_block_reader_names_irregular_input(tmp_path):
    """the file and one byte offset, counted from the start of the text whatever block the finding lies in"""
    err, _ = _through_blocks(tmp_path, b">a\nACGT\n>b\nAC\x00T\n>c\nAA\n", 12)
    assert err is not None and "a NUL byte at byte 13 of the text" in err and "in.fa" in err
    err, _ = _through_blocks(tmp_path, b"ACGT\n>a\nACGT\n", 64)
    assert err is not None and "before the first header line at byte 0 of the text" in err
    err, _ = _through_blocks(tmp_path, b">a\nACGT\n>b\n>c\nAC\n", 64)
    assert err is not None and "a record without sequence, its header at byte 8 of the text" in err
    text = FL.fasta([b"r%d" % i for i in range(40)], FL.sequences(40, 50, 4)) + b">empty\n>next\nAC\n"
    for block in (80, 128, 4096):
        err, _ = _through_blocks(tmp_path, text, block)
        assert err is not None and "its header at byte %d of the text" % text.index(b">empty") in err, (block, err)


def test_a_failed_decompressor_is_an_error_for_the_raw_reader(tmp_path):
    """biomcmc_read_compress keeps the check of biomcmc_getline_compress: a truncated .gz is not an end of data"""
    import gzip
    text = FL.fasta([b"r%d" % i for i in range(200)], FL.sequences(200, 300, 3))
    whole = gzip.compress(text)
    p = tmp_path / "cut.fa.gz"
    p.write_bytes(whole[:len(whole) // 2])
    err = FL.normalise_host(p, 4096, tmp_path / "o.fa")
    assert err is not None and "cut.fa.gz" in err and "decompressor reported an error" in err
    p.write_bytes(whole)
    assert FL.normalise_host(p, 4096, tmp_path / "o.fa") is None
    assert (tmp_path / "o.fa").read_bytes() == FL.normal_form(zip([b"r%d" % i for i in range(200)], FL.sequences(200, 300, 3)))


def test_sanitizer_program_compiles(tmp_path):
    """tools/fasta_blocks_check.c is the stand-alone host program (its own main, no GPU) for a sanitizer run of fasta_blocks.c over texts of its
    own making at several block sizes.  Like its siblings tools/uvdb_*_check.c it is run by hand, not by the suite; here it only has to compile.

      gcc -std=gnu11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iuvaia_amd/csrc/host -Iinclude tools/fasta_blocks_check.c \\
          uvaia_amd/csrc/host/fasta_blocks.c uvaia_amd/csrc/host/biomcmc_lite.c -lpthread -o /tmp/fasta_blocks_check && /tmp/fasta_blocks_check /tmp/fbc
    """
    host = os.path.join(ROOT, "uvaia_amd", "csrc", "host")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fasta_blocks_check.c"),
                           os.path.join(host, "fasta_blocks.c"), os.path.join(host, "biomcmc_lite.c"), "-lpthread", "-o", str(tmp_path / "fasta_blocks_check")])


def test_new_symbols_are_exported_and_the_header_stays_plain_c(tmp_path):
    lib = capi.load_library()
    new = ["uvaia_gpu_fasta_open", "uvaia_gpu_fasta_close", "uvaia_gpu_fasta_last_error", "uvaia_gpu_fasta_scan", "uvaia_gpu_fasta_records", "uvaia_gpu_fasta_rows",
           "uvaia_gpu_fasta_rows_host", "uvaia_gpu_fasta_bad", "uvaia_gpu_fasta_kernel_ms", "uvaia_gpu_fasta_chunk_bytes", "uvaia_gpu_fasta_pinned_alloc", "uvaia_gpu_fasta_pinned_free"]
    for name in new:
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    for m in ("scan", "records", "rows", "rows_host", "kernel_ms"):
        assert callable(getattr(capi.Fasta, m))
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_gpu.h"\n'
                   "int (*scan) (uvaia_gpu_fasta *, const void *, size_t, int, int *, size_t *) = uvaia_gpu_fasta_scan;\n"
                   "int (*rows) (uvaia_gpu_fasta *, int, const void **, size_t *, int *, int *) = uvaia_gpu_fasta_rows;\n"
                   "int main (void) { uvaia_gpu_fasta_record r; r.flags = UVAIA_GPU_FASTA_NUL | UVAIA_GPU_FASTA_EMPTY | UVAIA_GPU_FASTA_TEXT; return scan == 0 || rows == 0 || r.flags == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    n, cons = C.c_int(5), C.c_size_t(5)
    assert lib.uvaia_gpu_fasta_scan(None, None, 0, 1, C.byref(n), C.byref(cons)) == -1         # no handle: an error, not a fault
    assert lib.uvaia_gpu_fasta_chunk_bytes() % 16 == 0


def test_record_table_layout_matches_the_header(tmp_path):
    """the sibling of tests/test_abi.py::test_tuning_and_query_structs_match_the_header for uvaia_gpu_fasta_record"""
    fields = [f for f, _ in capi.FastaRecord._fields_]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uvaia_gpu.h"\nint main (void) { printf ("%zu", sizeof (uvaia_gpu_fasta_record));\n'
                   + "".join('printf (" %%zu", offsetof (uvaia_gpu_fasta_record, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(capi.FastaRecord) == capi.FASTA_RECORD_DTYPE.itemsize == 32
    assert got[1:] == [getattr(capi.FastaRecord, f).offset for f in fields] == [capi.FASTA_RECORD_DTYPE.fields[f][1] for f in fields]


def _refused(cmd, word, absent):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0, cmd
    assert word in r.stderr, (cmd, r.stderr[-2000:])
    assert b"HIP device" not in r.stderr, (cmd, r.stderr[-2000:])     # refused on its own grounds, not for the missing GPU
    for p in absent:
        assert not os.path.exists(p), (cmd, p)


def test_device_parse_refuses_option_conflicts_while_it_reads_them(tmp_path):
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">r0\nACGT\n")
    p = str(tmp_path / "o.uvdb")
    word = b"--device-parse reads FASTA text: it does not go with --merge, --unpack or --list"
    _refused([UVAIAPACK, "--device-parse", "--merge", "-o", p, str(fa)], word, [p])
    _refused([UVAIAPACK, "--device-parse", "--unpack", "-o", p, str(fa)], word, [p, p + ".aln.xz"])
    _refused([UVAIAPACK, "--device-parse", "--unpack", "--stdout", str(fa)], word, [p])
    _refused([UVAIAPACK, "--device-parse", "--list", str(fa)], word, [p])
    _refused([UVAIAPACK, "--device-parse", "--parse-block", "8", "-o", p, str(fa)], b"--parse-block: expected", [p])
    _refused([UVAIAPACK, "--parse-block", "4096", "-o", p, str(fa)], b"--parse-block sets the block size of --device-parse", [p])
