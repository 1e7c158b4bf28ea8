"""`uvaialign --device-parse` without a GPU: the new symbols, the plain C restatement of the A C G T count against a count in Python, the
record table's seq_len - non_n against the second counter of biomcmc_count_sequence_acgt, and what the command refuses before it touches
a GPU."""
import ctypes
import os
import re
import subprocess

import align_parse_lib as AP
import fasta_lib as FL
from uvaia_amd import align, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
NEW_GPU = ["uvaia_gpu_fasta_acgt", "uvaia_gpu_fasta_sequences", "uvaia_gpu_fasta_sequences_host", "uvaia_gpu_fasta_sequences_ms"]
NEW_ALIGN = ["uvaia_align_load_device"]


def _texts():
    return FL.corpus() + AP.alphabet_corpus() + [("edges", AP.edge_corpus()[0]), ("chunks", AP.chunk_corpus(4096))]


def test_the_new_symbols_are_declared_and_exported():
    gpu_h = open(os.path.join(ROOT, "include", "uvaia_gpu.h")).read()
    align_h = open(os.path.join(ROOT, "include", "uvaia_align.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "uvaia_amd", "lib", "libuvaia_gpu.so"))
    for s in NEW_GPU:
        assert re.search(r"\b%s\s*\(" % s, gpu_h) and s in capi.SYMBOLS and hasattr(lib, s), s
    for s in NEW_ALIGN:
        assert re.search(r"\b%s\s*\(" % s, align_h) and s in align.SYMBOLS and hasattr(lib, s), s
    host = ctypes.CDLL(os.path.join(ROOT, "uvaia_amd", "lib", "libuvaia_host.so"))
    assert hasattr(host, "fasta_count_acgt_host")
    assert re.search(r"\bfasta_count_acgt_host\s*\(", open(os.path.join(ROOT, "uvaia_amd", "csrc", "host", "fasta_blocks.h")).read())


def test_count_acgt_host_is_the_count_over_the_cleaned_sequence():
    seen = set()
    for label, text in _texts():
        rec, _ = FL.scan_host(text, final=True, max_records=4096)
        got = AP.count_acgt_host(text, rec)
        seqs = FL.clean_host(text, rec)
        assert got.tolist() == [AP.count_acgt_python(s) for s in seqs], label
        for s in seqs:
            seen.update(s)
    # the corpora hold what the count must tell apart: every invalid character, IUPAC codes, and lower case in the raw text
    assert set(AP.INVALID.upper()) <= seen and set(b"RYKMSWBDHV") <= seen
    assert all(any(c in text for _, text in _texts()) for c in (b"acgt", b"\r\n", b"n", b"x", b"o"))


def test_seq_len_minus_non_n_is_the_second_counter_and_acgt_the_first():
    n = 0
    for label, text in _texts():
        rec, _ = FL.scan_host(text, final=True, max_records=4096)
        acgt = AP.count_acgt_host(text, rec)
        for r, s, a in zip(rec, FL.clean_host(text, rec), acgt):
            frac = AP.count_sequence_acgt(s)
            ln = float(len(s)) if len(s) else 1.
            bad = int(r["seq_len"]) - int(r["non_n"])
            assert bad == sum(1 for c in s if c in AP.INVALID), label
            assert frac[2] == bad / ln and frac[0] == int(a) / ln, (label, frac, bad, a, ln)      # the very doubles the command's filters compare
            n += 1
    assert n > 200


def _refused(args):
    r = subprocess.run([UVAIALIGN, "-r", os.path.join(ROOT, "no_such_ref.fa")] + args + [os.path.join(ROOT, "no_such_seqs.fa")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    return r.returncode, r.stderr.decode()


def test_the_command_refuses_before_any_gpu_work():
    rc, err = _refused(["--parse-block", "65536"])
    assert rc == 1 and "--parse-block" in err and "needs that option" in err, err
    rc, err = _refused(["--device-parse", "--devices", "0,1"])
    assert rc == 1 and "--device-parse" in err and "ONE GPU" in err and "2 were listed" in err, err
    rc, err = _refused(["--device-parse", "--parse-block", "8"])
    assert rc == 1 and "--parse-block: expected 64 to 1073741824 bytes" in err, err
    help_text = subprocess.run([UVAIALIGN, "-h"], stdout=subprocess.PIPE, timeout=60).stdout.decode()
    assert "--device-parse" in help_text and "--parse-block" in help_text
