"""`uvaialign --device-parse` on a GPU box: the A C G T counts and the ragged sequences of the device parser against the plain C
restatements at the edges of fasta_sequences_kernel, uvaia_align_load_device against uvaia_align_load_block, and the command against
`uvaialign` without the option: text, standard output and both forms of the packed database, byte for byte."""
import gzip
import lzma
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_parse_lib as AP
import fasta_lib as FL
import fixtures as F
from uvaia_amd import align, capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIALIGN = os.path.join(ROOT, "bin", "uvaialign")
BLOCK = 256 << 10
JSON_LINE = r'device parse: \{"bytes": (\d+), "block_bytes": (\d+), "scan_ms": [0-9.]+, "count_ms": [0-9.]+, "sequences_ms": [0-9.]+, "align_ms": [0-9.]+\}'


@pytest.fixture(scope="module")
def parser():
    with capi.Fasta(BLOCK, 256) as f:
        yield f


def _at(text, off):
    """the text `off` bytes into a buffer whose start is 64-byte aligned"""
    raw = np.zeros(len(text) + off + 128, dtype=np.uint8)
    a = (-raw.ctypes.data) % 64
    buf = raw[a:a + off + len(text)]
    buf[off:] = np.frombuffer(text, dtype=np.uint8)
    assert buf.ctypes.data % 64 == 0
    return buf


def _reference(text):
    rec, consumed = FL.scan_host(text, final=True, max_records=256)
    return rec, consumed, FL.clean_host(text, rec), AP.count_acgt_host(text, rec)


def _check(f, seqs, sel, label):
    """fasta_sequences of a selection (None: all): offsets, every byte of the buffer, the guard"""
    ptr, off = f.sequences(sel)
    want = [seqs[k] for k in (range(len(seqs)) if sel is None else sel)]
    assert off.tolist() == [0] + np.cumsum([len(s) for s in want]).tolist(), label
    got, guard = f.sequences_host(off[-1])
    assert len(guard) == AP.GUARD and (guard == 0xEE).all(), (label, guard.tolist())
    if got != b"".join(want):
        bad = [k for k in range(len(want)) if got[off[k]:off[k + 1]] != want[k]]
        assert not bad, (label, bad[:5], got[off[bad[0]]:off[bad[0] + 1]][:40], want[bad[0]][:40])
    assert ptr != 0 or off[-1] == 0
    return off


@pytest.fixture(scope="module")
def edges():
    text, lengths = AP.edge_corpus()
    rec, consumed, seqs, acgt = _reference(text)
    assert [len(s) for s in seqs] == lengths and set(lengths) == set(AP.EDGE_LENGTHS) and consumed == len(text)
    return text, rec, seqs, acgt


def test_edge_lengths_at_every_destination_residue_and_every_misalignment(parser, edges):
    text, rec, seqs, acgt = edges
    for mis in range(16):
        n, _ = parser.scan(_at(text, mis), True, offset=mis)
        assert n == len(rec) and parser.records().tobytes() == rec.tobytes(), mis
        assert parser.acgt().tolist() == acgt.tolist(), mis
        off = _check(parser, seqs, None, ("all", mis))
        assert set((off[:-1] % 16).tolist()) == set(range(16))            # a sequence begins at every residue of a 16-byte piece
        assert {(int(a) % 16, int(b) % 16) for a, b in zip(off[:-1], off[1:])} >= {(0, 1), (15, 0), (1, 2), (0, 0)}
    ms = parser.sequences_ms()
    assert ms[0] > 0 and ms[1] > 0, ms


def test_selections(parser, edges):
    text, rec, seqs, acgt = edges
    n = len(rec)
    parser.scan(_at(text, 5), True, offset=5)
    for label, sel in (("every second", list(range(0, n, 2))), ("the odd ones", list(range(1, n, 2))), ("the last", [n - 1]), ("reversed", list(range(n - 1, -1, -1))),
                       ("the first three", None)):
        if sel is None:
            ptr, off = parser.sequences(None, n_sel=3)
            got, guard = parser.sequences_host(off[-1])
            assert got == b"".join(seqs[:3]) and (guard == 0xEE).all(), label
        else:
            _check(parser, seqs, sel, label)
    # nothing selected: no byte, the guard alone
    ptr, off = parser.sequences([])
    assert off.tolist() == [0]
    got, guard = parser.sequences_host(0)
    assert got == b"" and (guard == 0xEE).all()


def test_a_bad_selection_is_refused_and_the_handle_works_afterwards(parser, edges):
    text, rec, seqs, acgt = edges
    n = len(rec)
    parser.scan(_at(text, 0), True)
    for sel, what in (([0, 3, 3], "twice"), ([1, n], "%d records" % n), ([-1], "%d records" % n), (list(range(n)) + [0], "")):
        with pytest.raises(capi.GpuError) as g:
            parser.sequences(sel)
        assert g.value.code == -1 and what in str(g.value), (sel[:4], str(g.value))
        with pytest.raises(capi.GpuError):                                # no buffer is handed out after a refusal
            parser.sequences_host(0)
        _check(parser, seqs, [2, 0], "after a refusal")
    assert parser.acgt().tolist() == acgt.tolist()


def test_bodies_across_chunks_and_a_header_across_a_chunk_boundary(parser):
    chunk = capi.load_library().uvaia_gpu_fasta_chunk_bytes()
    text = AP.chunk_corpus(chunk)
    rec, consumed, seqs, acgt = _reference(text)
    spans = [(int(r["body_off"]) // chunk, (int(r["body_off"]) + int(r["body_len"]) - 1) // chunk) for r in rec]
    assert spans[0][1] - spans[0][0] == 1 and spans[1][1] - spans[1][0] == 2          # two chunks, three chunks
    assert int(rec[3]["name_off"]) // chunk < (int(rec[3]["name_off"]) + int(rec[3]["name_len"])) // chunk
    for mis in (0, 7, 15):
        n, c = parser.scan(_at(text, mis), True, offset=mis)
        assert (n, c) == (len(rec), consumed) and parser.records().tobytes() == rec.tobytes()
        assert parser.acgt().tolist() == acgt.tolist(), mis
        _check(parser, seqs, None, ("chunks", mis))
        _check(parser, seqs, [4, 1, 3], ("chunks, some", mis))


def test_counts_over_the_parser_corpora(parser):
    chunk = capi.load_library().uvaia_gpu_fasta_chunk_bytes()
    for label, text in FL.shape_corpus() + FL.ragged_corpus(chunk) + AP.alphabet_corpus():
        rec, consumed, seqs, acgt = _reference(text)
        n, _ = parser.scan(_at(text, 3), True, offset=3)
        assert n == len(rec) and parser.acgt().tolist() == acgt.tolist(), label
        _check(parser, seqs, None, label)


# ------------------------------------------------------------------------------------------------------------------ uvaia_align_load_device
@pytest.fixture(scope="module")
def pool():
    """a reference of 1 000 sites, 200 unaligned sequences, and the scores and rows of uvaia_align_load_block"""
    ref, seqs = _pool_inputs()
    with align.Aligner(ref) as al:
        al.load(seqs)
        al.run()
        score, rows = al.fetch()
    return ref, seqs, score.copy(), rows.copy()


def _pool_inputs():
    ref = F.random_acgt(1000, 41)
    return ref, F.unaligned_queries(ref, 200, 42, p_indel=0.002, n_runs=(20, 20, 60))


# (a worker process: the runtime a torch wheel brings along finds the GPU only if it is loaded before the library's, tests/test_rows_gpu.py)
TORCH_WORKER = r"""
import sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, root + "/tests")
import numpy as np
import torch
torch.cuda.init()                                     # the tensor's runtime first, the aligner's after it
import test_align_parse_gpu as T
from uvaia_amd import align
ref, seqs = T._pool_inputs()
blob = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
t = torch.from_numpy(blob).to("cuda:0")
torch.cuda.synchronize()
with align.Aligner(ref) as al:
    al.load(seqs); al.run()
    score, rows = (x.copy() for x in al.fetch())
    al.load_device(t.data_ptr(), off); al.run()
    s2, r2 = al.fetch()
    assert np.array_equal(s2, score) and np.array_equal(r2, rows)
    al.load_device(t.data_ptr(), off[50:121]); al.run()          # a part of the pool, by offsets that do not begin at 0
    s3, r3 = al.fetch()
    assert np.array_equal(s3, score[50:120]) and np.array_equal(r3, rows[50:120])
    for bad in (blob.ctypes.data, t.cpu().data_ptr()):           # host pointers are refused, and the aligner works afterwards
        try:
            al.load_device(bad, off)
            raise SystemExit("a host pointer was accepted")
        except align.AlignError as e:
            assert e.code == -1 and "device" in str(e), str(e)
        al.load(seqs[:40]); al.run()
        s4, r4 = al.fetch()
        assert np.array_equal(s4, score[:40]) and np.array_equal(r4, rows[:40])
    al.load_device(t.data_ptr(), off[:1]); al.run()              # an empty pool
    assert al.n == 0
print("TENSOR OK")
"""


def test_load_device_from_a_torch_tensor(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(TORCH_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"TENSOR OK" in r.stdout, r.stderr[-3000:]


def test_load_device_from_the_parsers_buffer(pool, parser):
    ref, seqs, score, rows = pool
    text = b"".join(AP._shape(i, b"s%d" % i, s) for i, s in enumerate(seqs))
    assert len(text) < BLOCK
    n, _ = parser.scan(_at(text, 9), True, offset=9)
    assert n == len(seqs)
    ptr, off = parser.sequences()
    assert off[-1] == sum(len(s) for s in seqs)
    with align.Aligner(ref) as al:
        al.load_device(ptr, off)
        al.run()
        s2, r2 = al.fetch()
        assert np.array_equal(s2, score) and np.array_equal(r2, rows)
        # a range that ends beyond the allocation the bytes lie in is refused, and the aligner works afterwards
        beyond = off.copy()
        beyond[-1] += 1 << 24
        with pytest.raises(align.AlignError) as e:
            al.load_device(ptr, beyond)
        assert e.value.code == -1 and "beyond" in str(e.value)
        al.load(seqs[100:])
        al.run()
        s3, r3 = al.fetch()
        assert np.array_equal(s3, score[100:]) and np.array_equal(r3, rows[100:])
    sel = list(range(199, -1, -3))                                       # a selection, in another order
    ptr, off = parser.sequences(sel)
    with align.Aligner(ref) as al:
        al.load_device(ptr, off)
        al.run()
        s4, r4 = al.fetch()
        assert np.array_equal(s4, score[sel]) and np.array_equal(r4, rows[sel])


# ------------------------------------------------------------------------------------------------------------------ the command
def _run_together(cmds):
    """[(return code, stdout, stderr)] of the commands, eight at a time"""
    out = []
    for a in range(0, len(cmds), 8):
        procs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for c in cmds[a:a + 8]]
        try:
            for p in procs:
                o, err = p.communicate(timeout=600)
                out.append((p.returncode, o, err.decode(errors="replace")))
        finally:                                               # a timeout (or any other way out) leaves none of the batch running
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.communicate()
        died = [(c, r[0]) for c, r in zip(cmds[a:a + 8], out[a:]) if r[0] < 0 or r[0] in (124, 134, 137, 139)]
        assert not died, died[:2]                              # a command that was killed: nothing more is started
    return out


REF_LEN = 1200


def _threshold_record(ref, n_acgt):
    """a sequence of the reference's length with exactly n_acgt A C G T sites, the others IUPAC codes (no N: the ACGT filter alone decides)"""
    s = bytearray(ref)
    for i in range(len(s) - n_acgt):
        s[len(s) - 1 - i] = b"RYKM"[i % 4]
    assert AP.count_acgt_python(s) == n_acgt
    return bytes(s)


@pytest.fixture(scope="module")
def commands(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_parse")
    ref = F.random_acgt(REF_LEN, 51)
    seqs = F.unaligned_queries(ref, 600, 52, p_indel=0.002, n_runs=(20, 20, 60))
    names = ["hCoV-19/seq %d|2021-0%d" % (i, 1 + i % 9) for i in range(len(seqs))]
    # what each filter drops (-a 0.5: N etc. above 0.5, ACGT below 0.45), and the records next to its thresholds that stay
    edge = int(np.ceil(0.45 * REF_LEN - 1e-9))                            # the fewest A C G T sites that pass at the reference's length
    special = {7: ("too short", ref[:REF_LEN * 2 // 3 - 1]), 8: ("shortest kept", ref[:REF_LEN * 2 // 3]), 99: ("too long", ref + ref[:REF_LEN // 2 + 1]),
               100: ("longest kept", ref + ref[:REF_LEN // 2]), 250: ("too many N", b"N" * (REF_LEN // 2 + 1) + ref[REF_LEN // 2 + 1:]),
               251: ("N at the threshold", b"N" * (REF_LEN // 2) + ref[REF_LEN // 2:]), 400: ("ACGT one below", _threshold_record(ref, edge - 1)),
               401: ("ACGT at the threshold", _threshold_record(ref, edge)), 402: ("ACGT one above", _threshold_record(ref, edge + 1)), 599: ("too short at the end", b"ACGTN")}
    for i, (nm, s) in special.items():
        names[i], seqs[i] = nm, s
    lower = [s.lower() if i % 5 == 1 else s for i, s in enumerate(seqs)]
    nb = [n.encode() for n in names]
    texts = {"one_line": [FL.fasta(nb, lower)], "wrap60": [FL.fasta(nb, seqs, wrap=60)], "crlf": [FL.fasta(nb, seqs, wrap=70, eol=b"\r\n")],
             "gz": [FL.fasta(nb, seqs, wrap=60)], "two_files": [FL.fasta(nb[:333], seqs[:333], wrap=60), FL.fasta(nb[333:], lower[333:], last_eol=False)]}
    paths = {}
    for tag, parts in texts.items():
        paths[tag] = []
        for i, t in enumerate(parts):
            p = d / ("%s_%d.fa%s" % (tag, i, ".gz" if tag == "gz" else ""))
            with (gzip.open if tag == "gz" else open)(p, "wb") as fh:
                fh.write(t)
            paths[tag].append(str(p))
    (d / "ref.fa").write_bytes(b">the reference\n" + ref + b"\n")
    # an input with a header without sequence, far enough in for a block of 64 KiB to have been aligned before
    bad_at = len(FL.fasta(nb[:300], seqs[:300], wrap=60))
    (d / "empty_record.fa").write_bytes(FL.fasta(nb[:300], seqs[:300], wrap=60) + b">a header without sequence\n" + FL.fasta(nb[300:320], seqs[300:320], wrap=60))

    cases = [("one_line", []), ("wrap60", []), ("crlf", []), ("gz", []), ("two_files", []), ("wrap60", ["-p", "7", "--parse-block", "65536"]), ("two_files", ["-p", "4096"])]
    cmds, keys = [], []
    for tag, extra in cases:
        key = tag + "".join(extra).replace("-", "_")
        for route, opt in (("default", []), ("parse", ["--device-parse"])):
            ex = [e for e in extra if route == "parse" or e not in ("--parse-block", "65536")]
            base = [UVAIALIGN, "-r", str(d / "ref.fa")] + opt + ex + paths[tag]
            stem = str(d / ("%s.%s" % (key, route)))
            for out, how in ((["-o", stem], "text"), (["--stdout"], "stdout"), (["--packed", stem + ".uvdb"], "packed"), (["--packed", stem + ".c.uvdb", "--compact"], "compact")):
                if how in ("text", "packed") or not extra:            # (the cases with options of their own: the text and the dense file)
                    cmds.append(base + out)
                    keys.append((key, route, how))
    cmds.append([UVAIALIGN, "-r", str(d / "ref.fa"), "--device-parse", "--parse-block", "65536", "-p", "50", "-o", str(d / "empty_record"), str(d / "empty_record.fa")])
    keys.append(("empty_record", "parse", "text"))
    res = dict(zip(keys, _run_together(cmds)))
    return d, res, names, seqs, bad_at


def _dropped(err):
    return [ln for ln in err.split("\n") if ln.startswith("Sequence ") and (" has size too different" in ln or " has proportion of " in ln)]


def _pair(res, key, how):
    a, b = res[(key, "default", how)], res[(key, "parse", how)]
    assert a[0] == 0, a[2][-3000:]
    assert b[0] == 0, b[2][-3000:]
    m = re.search(JSON_LINE, b[2])
    assert m and int(m.group(1)) > 0, b[2][-1500:]                       # the option was taken: the line of the new route is there ...
    assert not re.search(JSON_LINE, a[2])                                # ... and only there
    assert _dropped(a[2]) == _dropped(b[2]) and len(_dropped(a[2])) >= 5
    return a, b


KEYS = ("one_line", "wrap60", "crlf", "gz", "two_files")


def test_the_input_covers_what_it_should(commands):
    d, res, names, seqs, _ = commands
    rc, _, err = res[("one_line", "default", "text")]
    assert rc == 0
    out_names, rows = F.read_fasta_bytes(lzma.open(str(d / "one_line.default.aln.xz"), "rb").read())
    assert 0 < len(rows) < len(seqs) and all(len(r) == REF_LEN for r in rows)
    gone = set(names) - set(out_names)
    assert gone == {"too short", "too long", "too many N", "ACGT one below", "too short at the end"}, gone
    lines = "\n".join(_dropped(err))
    for name, why in (("too short", "size too different"), ("too long", "size too different"), ("too many N", "proportion of N etc."), ("ACGT one below", "proportion of ACGT")):
        assert re.search(r"Sequence %s has %s" % (name, why), lines), (name, lines)
    assert sum(1 for s in seqs if len(s) != REF_LEN) > 300               # ragged: insertions and deletions


@pytest.mark.parametrize("key", KEYS)
def test_text_output_is_the_default_routes(commands, key):
    d, res, *_ = commands
    _pair(res, key, "text")
    a, b = (lzma.open(str(d / ("%s.%s.aln.xz" % (key, r))), "rb").read() for r in ("default", "parse"))
    assert a == b and a.count(b">") > 500


@pytest.mark.parametrize("key", KEYS)
def test_stdout_is_the_default_routes(commands, key):
    d, res, *_ = commands
    a, b = _pair(res, key, "stdout")
    assert a[1] == b[1] and a[1].count(b">") > 500
    assert a[1] == lzma.open(str(d / ("%s.default.aln.xz" % key)), "rb").read()


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("how", ["packed", "compact"])
def test_packed_database_is_the_default_routes(commands, key, how):
    d, res, *_ = commands
    _pair(res, key, how)
    suffix = ".uvdb" if how == "packed" else ".c.uvdb"
    a, b = ((d / ("%s.%s%s" % (key, r, suffix))).read_bytes() for r in ("default", "parse"))
    assert a == b and len(a) > 4096


@pytest.mark.parametrize("key", ["wrap60_p7__parse_block65536", "two_files_p4096"])
def test_pools_cut_scans_and_scans_cut_records(commands, key):
    d, res, *_ = commands
    _, b = _pair(res, key, "text")
    _pair(res, key, "packed")
    m = re.search(JSON_LINE, b[2])
    if "65536" in key:
        assert int(m.group(2)) == 65536 and int(m.group(1)) > 8 * 65536      # several blocks, each cutting a record
    for suffix in (".aln.xz", ".uvdb"):
        a, b = (d / ("%s.default%s" % (key, suffix))).read_bytes(), (d / ("%s.parse%s" % (key, suffix))).read_bytes()
        if suffix == ".aln.xz":
            a, b = lzma.decompress(a), lzma.decompress(b)
        assert a == b and len(a) > 4096
    assert lzma.open(str(d / ("%s.parse.aln.xz" % key)), "rb").read() == lzma.open(str(d / "wrap60.default.aln.xz"), "rb").read()


def test_a_header_without_sequence_ends_the_command(commands):
    d, res, names, seqs, bad_at = commands
    rc, _, err = res[("empty_record", "parse", "text")]
    assert rc not in (0, None) and rc > 0, err[-2000:]
    assert "empty_record.fa: FASTA text: a record without sequence, its header at byte %d of the text" % bad_at in err, err[-2000:]
    assert "`uvaialign` without it reads this file line by line" in err
    out_names, rows = F.read_fasta_bytes(lzma.open(str(d / "empty_record.aln.xz"), "rb").read())      # what was aligned before: a complete file
    assert 0 < len(rows) < 300 and out_names == [n for n in names[:300] if n in set(out_names)] and all(len(r) == REF_LEN for r in rows)
