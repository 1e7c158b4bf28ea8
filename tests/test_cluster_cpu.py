"""CPU checks of uvaiaclust: hand-worked answers of the restatement (each pins one quirk of the reference's code), the C restatement
against a Python transcription of the reference's loops, the C ABI (plain C, exported, no CPU path) and the command line's refusals."""
import os
import random
import re
import subprocess

import pytest

import cluster_lib as CL
from uvaia_amd import capi, cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UVAIACLUST = os.path.join(ROOT, "bin", "uvaiaclust")


def _sub(base, sites, ch):
    s = bytearray(base)
    for i in sites:
        s[i] = ord(ch)
    return bytes(s)


def _both(ref, seqs, queues, dist, trim, n_score, n_queues):
    got = CL.rs_cluster(ref, seqs, queues, dist, trim, n_score, n_queues)
    py = CL.py_cluster(ref, seqs, queues, dist, trim, n_score, n_queues)
    assert got[0] == py[0] and got[1].tolist() == py[1].tolist()
    return got


# ------------------------------------------------------------------------------------------------------------- known answers
def test_n_counts_as_a_difference():
    ref = b"A" * 20
    seqs = [ref, b"A" * 19 + b"N"]
    cl, sc = _both(ref, seqs, [0, 0], 0, 0, 1, 1)
    assert cl == [(1, []), (0, [])]                     # two clusters at d = 0: N against A counts
    assert sc.tolist() == [[1, 19, 20], [0, -1, 20]]
    cl, _ = _both(ref, seqs, [0, 0], 1, 0, 1, 1)
    assert cl == [(0, [1])]


def test_stored_d_plus_one_makes_a_sequence_found_its_own_cluster():
    ref = b"A" * 40
    s0 = _sub(ref, range(0, 10), "C")                   # r = 10: medoid, stored 10
    s1 = _sub(ref, range(20, 31), "G")                  # r = 11: compared with s0, fails: medoid, stored d + 1 = 2
    s2 = _sub(s1, [31], "G")                            # r = 12, one site from s1, but outside both rings (10 and 2)
    cl, sc = _both(ref, [s0, s1, s2], [0, 0, 0], 1, 0, 0, 1)
    assert cl == [(2, []), (0, []), (1, [])]
    assert sc.tolist() == [[12, 40], [10, 40], [2, 40]]


def test_first_member_stays_medoid():
    ref = b"A" * 20
    s0 = _sub(ref, [0, 1], "N")
    s1 = _sub(ref, [0], "N")                            # fewer Ns, joins s0, which stays the medoid
    cl, sc = _both(ref, [s0, s1], [0, 0], 1, 0, 1, 1)
    assert cl == [(0, [1])]
    assert sc.tolist() == [[2, 0, 20]]


def test_tail_window_counts_under_trim():
    ref = b"A" * 30
    s0 = _sub(ref, [10], "C")                           # r = 1, p = 7 (relative to trim 3)
    s1 = _sub(ref, [10, 28], "C")                       # same inside [3, 27); site 28 lies in the window [9, 33) of the comparison
    cl, sc = _both(ref, [s0, s1], [0, 0], 0, 3, 1, 1)
    assert cl == [(0, []), (1, [])]
    assert sc.tolist() == [[1, 7, 30], [1, 7, 30]]
    cl, _ = _both(ref, [s0, _sub(ref, [10, 2], "C")], [0, 0], 0, 3, 1, 1)   # a difference in the head is not in the window
    assert cl == [(0, [1])]


def test_round_robin_restarts_at_queue_zero_per_file():
    assert CL.round_robin([3, 2], 2) == [0, 1, 0, 0, 1]
    assert cluster.queues_round_robin([3, 2], 2).tolist() == [0, 1, 0, 0, 1]
    ref = b"A" * 20
    seqs = [ref] * 5
    cl, _ = _both(ref, seqs, CL.round_robin([3, 2], 2), 0, 0, 1, 2)
    assert cl == [(0, [2, 3, 1, 4])]
    cl, _ = _both(ref, seqs, CL.round_robin([5], 2), 0, 0, 1, 2)
    assert cl == [(0, [2, 4, 1, 3])]


def test_merge_windows_and_splice_order():
    ref = b"A" * 40
    o0 = _sub(ref, range(0, 5), "C")                    # queue 0, stored 5
    o1 = _sub(ref, [20, 21], "G")                       # queue 1, stored 2
    o2 = _sub(ref, range(10, 13), "C")                  # queue 0, stored 3
    o3 = _sub(o0, [39], "T")                            # queue 1, stored 6, one site from o0
    o4 = o0                                             # queue 0, joins o0
    o5 = _sub(ref, range(10, 14), "C")                  # queue 1, stored 4, one site from o2
    seqs = [o0, o1, o2, o3, o4, o5]
    cl, sc = _both(ref, seqs, CL.round_robin([6], 2), 1, 0, 0, 2)
    # queue 1 sorted: o3 (6) joins o0 after o4, o5 (4) joins o2, o1 (2) is appended
    assert cl == [(0, [4, 3]), (2, [5]), (1, [])]
    assert sc.tolist() == [[5, 40], [3, 40], [2, 40]]


def test_final_tie_order():
    ref = b"A" * 20
    s0, s1, s2 = _sub(ref, [0], "C"), _sub(ref, [5], "C"), _sub(ref, [9], "C")
    cl, sc = _both(ref, [s0, s1, s2, s2], [0] * 4, 0, 0, 0, 1)
    assert cl == [(2, [3]), (0, []), (1, [])]           # equal score vectors keep their order
    assert sc.tolist() == [[1, 20]] * 3


def test_empty_queue_merges_as_a_no_op():
    ref = b"A" * 20
    cl, _ = _both(ref, [ref, ref], [0, 1], 0, 0, 1, 4)
    assert cl == [(0, [1])]
    cl, _ = _both(ref, [ref], [0], 0, 0, 1, 3)
    assert cl == [(0, [])]
    cl, _ = _both(ref, [ref, ref], [1, 1], 0, 0, 1, 2)   # an empty absorbing queue takes the other list
    assert cl == [(0, [1])]


def test_reference_from_records():
    assert CL.rs_reference([b"ANNTN-", b"ACNTGN", b"TTTAAA"]) == b"ACTTGA"    # Ns filled by later records, the rest becomes A
    assert CL.rs_reference([b"ACGTAC", b"TTTTTT"]) == b"ACGTAC"              # no N left: later records do not count


# --------------------------------------------------------------------------------------------------------- C against Python
def _random_case(rng):
    nchar = rng.randint(20, 60)
    alphabet = b"ACGTN-" * 4 + b"RYKMSWBDHVacgtn"
    root = bytes(rng.choice(b"ACGT") for _ in range(nchar))
    fams = [bytearray(root) for _ in range(rng.randint(1, 4))]
    for f in fams:
        for _ in range(rng.randint(0, 6)):
            f[rng.randrange(nchar)] = rng.choice(alphabet)
    n_files = rng.randint(1, 3)
    sizes = [rng.randint(0, 12) for _ in range(n_files)]
    if not sum(sizes):
        sizes[0] = 1
    seqs = []
    for _ in range(sum(sizes)):
        s = bytearray(rng.choice(fams))
        for _ in range(rng.randint(0, 3)):
            s[rng.randrange(nchar)] = rng.choice(alphabet)
        if rng.random() < 0.3:
            a = rng.randrange(nchar)
            b = min(nchar, a + rng.randint(1, 8))
            s[a:b] = b"N" * (b - a)
        seqs.append(bytes(s[:nchar]))
    n_queues = rng.randint(1, 9)
    dist, trim, n_score = CL.clamp(nchar, rng.randint(0, 4), rng.randint(0, 6), rng.randint(0, 3))
    ref = CL.rs_reference(seqs[:1024]) if rng.random() < 0.5 else bytes(rng.choice(b"ACGT") for _ in range(nchar))
    return ref, seqs, CL.round_robin(sizes, n_queues), dist, trim, n_score, n_queues


def test_c_restatement_equals_python_transcription():
    rng = random.Random(20261016)
    for case in range(300):
        ref, seqs, queues, dist, trim, n_score, n_queues = _random_case(rng)
        got = CL.rs_cluster(ref, seqs, queues, dist, trim, n_score, n_queues)
        want = CL.py_cluster(ref, seqs, queues, dist, trim, n_score, n_queues)
        assert got[0] == want[0], "case %d: clusters differ" % case
        assert got[1].tolist() == want[1].tolist(), "case %d: scores differ" % case


# ------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.load_library()


def test_cluster_header_symbols_all_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "uvaia_cluster.h")).read()
    declared = set(re.findall(r"\b(uvaia_clust_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(cluster.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name


def test_cluster_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "uvaia_cluster.h"\nint main(void){ uvaia_clust_ctx *c = 0; (void)c; return UVAIA_GPU_OK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def test_cluster_refuses_to_run_without_a_gpu():
    _no_gpu()
    with pytest.raises(cluster.ClusterError) as ei:
        cluster.Clusterer(b"ACGTACGTAC", dist=1)
    assert ei.value.code == -2          # UVAIA_GPU_ENODEV: there is no CPU path


def _fasta(path, recs):
    with open(path, "wb") as fh:
        for n, s in recs:
            fh.write(b">" + n + b"\n" + s + b"\n")


def test_cli_without_gpu_fails_loudly(tmp_path):
    _no_gpu()
    f = tmp_path / "a.fa"
    _fasta(f, [(b"s1", b"ACGTACGTACGT"), (b"s2", b"ACGTACGTACGA")])
    r = subprocess.run([UVAIACLUST, "-o", str(tmp_path / "o"), str(f)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "gfx950" in (r.stdout + r.stderr) or "HIP device" in (r.stdout + r.stderr)
    assert not (tmp_path / "o.csv.xz").exists()


def test_cli_refuses_high_bytes(tmp_path):
    f = tmp_path / "a.fa"
    _fasta(f, [(b"s1", b"ACGTACGTACGT"), (b"s2", b"ACGTAC\xc3TACGT")])
    r = subprocess.run([UVAIACLUST, "-o", str(tmp_path / "o"), str(f)], capture_output=True, text=True, errors="replace")
    assert r.returncode != 0
    assert "s2" in r.stderr + r.stdout and "0xc3" in r.stderr + r.stdout


def test_cli_refuses_length_mismatch(tmp_path):
    f, g = tmp_path / "a.fa", tmp_path / "ref.fa"
    _fasta(f, [(b"s1", b"ACGTACGTACGT"), (b"s2", b"ACGTACGTACGA"), (b"s3", b"ACGTACGTACG")])
    _fasta(g, [(b"ref", b"ACGTACGTACGT")])
    r = subprocess.run([UVAIACLUST, "-r", str(g), "-o", str(tmp_path / "o"), str(f)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "s3" in r.stderr + r.stdout and "unaligned" in r.stderr + r.stdout
