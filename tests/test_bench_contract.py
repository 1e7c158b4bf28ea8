"""bench.py on a box without a GPU: it must refuse to run (the engine has no CPU path) rather than time something else, and its
command line must keep the driver's contract (--gpus/--steps/--warmup, defaults that finish in minutes).  On the MI355X: what a
plain run prints and what --dump-outputs writes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_and_defaults():
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert (a.gpus, a.queries, a.refs, a.nbest, a.mode) == (1, 1000, 100000, 100, "iupac") and a.steps <= 10 and a.warmup >= 1
        assert not a.full and a.dump_outputs is None           # a plain run: the headline alone, nothing written
        sys.argv = ["bench.py", "--gpus", "8", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        assert (a.gpus, a.steps, a.warmup) == (8, 7, 2)
        sys.argv = ["bench.py", "--full", "--dump-outputs", "out"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "out"
        sys.argv = ["bench.py", "--gpus", "2", "--dump-outputs", "out"]      # the heaps of one process only
        with pytest.raises(SystemExit):
            bench.parse()
    finally:
        sys.argv = argv


def test_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "no CPU path" in (p.stderr + p.stdout)
    assert not p.stdout.strip().startswith("{")          # no result line


@pytest.mark.gpu
def test_plain_run_dumps_the_heaps_of_its_last_timed_step(tmp_path):
    """A plain run prints the headline alone; --dump-outputs leaves the heaps of the last timed step, best first, equal to the
    oracle's search of the same seeded inputs."""
    import json
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import oracle_lib as O
    from uvaia_amd import hostlib
    nq, n_ref, nbest, pool = 40, 3000, 10, 1024
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--queries", str(nq),
                        "--refs", str(n_ref), "--nbest", str(nbest), "--pool", str(pool), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 3 and len(out["step_ms_rank0"]) == 3 and out["ms_per_step"] > 0
    assert out["sweep"] is None and out["cpu_baseline"] is None and out["parity_check_on_timed_path"] is None
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("query_index", "n_items", "max_incompatible", "scores", "ordinals")}
    assert all(a.dtype == np.float64 for a in got.values())

    gen = hostlib.Synth(29903, seed=20241008, preset=0)
    qseqs, _ = gen.generate_bytes(bench.QUERY_INDEX0, nq)
    refs, _ = gen.generate_bytes(0, n_ref)
    oq = O.Query(qseqs, ["query_%d" % i for i in range(nq)])
    gold = O.search(oq, refs, ["ref_%d" % i for i in range(n_ref)], pool=pool, nbest=nbest, ambig_r=0.5)
    assert list(got["query_index"]) == list(range(oq.ntax))
    assert list(got["max_incompatible"]) == gold.final_T
    for iq in range(oq.ntax):
        k = int(got["n_items"][iq])
        assert k == len(gold.rows[iq])
        assert [(tuple(int(v) for v in s), int(o)) for s, o in zip(got["scores"][iq, :k], got["ordinals"][iq, :k])] == \
               [(tuple(s), o) for o, _, s in gold.rows[iq]], "query %d" % iq
        assert (got["scores"][iq, k:] == -1).all() and (got["ordinals"][iq, k:] == -1).all()
