"""The inputs of tests/scan_edges.py through the two-counter pair scans on the MI355X (`pytest -m gpu`), by uvaia_gpu_shard_scan on a plain context:
the call goes straight to launch_scan2 and leaves the raw counters cnt[query][column] (first | second << 16), the bounds tmin[query][tile] and the
aux block (valid sites, consensus pre-score) in buffers of the caller.  (uvaia_gpu_last_batch_scores recounts a batch with the four-counter kernel,
so the all-pairs tests of test_gpu_parity.py never see these counters.)  Every comparison is equality with scan_edges.plain_count, over every
real query and every reference of the range.  The buffers are torch device tensors filled with a sentinel, with a guard tail: rows the launch does
not cover and the tail must keep it (the scans run in a worker process, which loads torch's runtime before the engine's).  After uvaia_gpu_db_rederive the same scan must give the same bytes.  The stream tests decode query tables 7, 8
and 10 and compare them with the model of scan_edges.py; they judge no count.

The instantiations launch_scan2 can launch, and the runs that select them (scan_edges.tuning):
  scan3_kernel<4, false|true, 1>   scan: compressed, scan_waves_per_block 4, scan_tiles_per_wave 1      ids *-nw4r1
  scan3_kernel<4, false|true, 2>   scan: compressed, scan_waves_per_block 4, scan_tiles_per_wave 2      ids *-nw4r2
  scan3_kernel<8, false|true, 1>   scan: compressed, scan_waves_per_block 8, scan_tiles_per_wave 1      ids *-nw8r1
  scan3_kernel<8, false|true, 2>   scan: compressed (the defaults)                                      ids *-nw8r2
  scan3_kernel<8, false|true, 4>   scan: compressed, scan_waves_per_block 8, scan_tiles_per_wave 4      ids *-nw8r4
  scan2_iupac_kernel<QT, CONS>, scan2_acgt_kernel<QT, CONS>, QT = 1, 2, 4, 8, 16, CONS = true, false    scan: packed with 1, 2, 3, 5 / 8, 9 / 17 / 32
                                   queries (group K); CONS = false: the prepared query with idx_c moved into idx_m (ids *-nocons); C3 reaches
                                   scan2_acgt_kernel<8, true> by the fallback of host_qtables.inc
false|true is --acgt: ids *-iupac-* and *-acgt-*."""
import atexit
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scan_edges as SE                       # noqa: E402
from uvaia_amd import capi                    # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 2048                 # dwords behind the last row of every buffer


def cases(*groups):
    runs = [r for g in groups for r in SE.runs(g)]
    return pytest.mark.parametrize("key,acgt,v,cons", runs, ids=[SE.run_id(*r) for r in runs])


def engine_query(key, acgt, cons):
    q = SE.query(key, acgt)
    if cons:
        return q
    # no constant-and-complete column: the counters do not depend on the split of the columns, the CONS = false kernels are the ones launched
    return types.SimpleNamespace(seqs=q.seqs, consensus=q.consensus, idx_c=np.zeros(0, dtype=np.int64), idx_m=np.sort(np.concatenate([q.idx_c, q.idx_m])),
                                 idx=q.idx, trim=q.trim, acgt=q.acgt, ntax=q.ntax)


def shard_scan(eng, first, n):
    """one uvaia_gpu_shard_scan into sentinel-filled device tensors: (cnt [rows, cols] uint32, tmin [rows, tiles, 2], aux int32, the three guard tails)"""
    import torch
    rows, tiles = eng.shard_rows(), (first + n + 63) // 64 - first // 64
    sizes = (rows * tiles * 64, rows * tiles * 2, eng.shard_aux_bytes(tiles) // 4)
    bufs = [torch.full((s + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for s in sizes]
    torch.cuda.synchronize()
    eng.shard_scan(first, n, *[b.data_ptr() for b in bufs])
    eng.scan_wait()
    host = [b.cpu().numpy() for b in bufs]
    tails = [h[s:] for h, s in zip(host, sizes)]
    return host[0][:sizes[0]].view(np.uint32).reshape(rows, tiles * 64), host[1][:sizes[1]].reshape(rows, tiles, 2), host[2][:sizes[2]], tails


def check_scan(key, acgt, q, eng, db_n, first, n):
    case = SE.CASES[key]
    gfirst, gsecond, gvalid, gpre = SE.gold(key, acgt)
    cnt, tmin, aux, tails = shard_scan(eng, first, n)
    what = (key, "acgt" if acgt else "iupac", db_n, first, n)
    t0, tiles = first // 64, tmin.shape[1]
    a0, a1 = case.active or (0, q.ntax)
    # 1. counters: every real pair of the range
    want = gfirst[a0:a1, first:first + n].astype(np.uint32) | (gsecond[a0:a1, first:first + n].astype(np.uint32) << 16)
    got = cnt[a0:a1, first - t0 * 64:first - t0 * 64 + n]
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "pairs that differ: %d, first (query, column) %s got %#x want %#x" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))
    # 2. bounds
    assert np.array_equal(tmin[a0:a1], SE.plain_bounds(gfirst, gsecond, acgt, first, n)[a0:a1]), what
    # 3. valid sites and the consensus pre-score of the references in the tiles the range touches
    r0, r1 = t0 * 64, min(db_n, (t0 + tiles) * 64)
    assert np.array_equal(aux[:r1 - r0], gvalid[r0:r1]), what
    if len(q.idx_c):
        rt = aux[tiles * 64:].reshape(tiles * 64, 4)
        assert np.array_equal(rt[:r1 - r0, 0], gpre[0][r0:r1]) and np.array_equal(rt[:r1 - r0, 1 if acgt else 3], gpre[1][r0:r1]), what
    else:
        assert aux.size == tiles * 64
    # 4. sentinels: rows the launch does not cover, and the guard tails
    w0, w1 = SE.written_rows(q.ntax, eng.scan_variant(), case.active)
    for a in (cnt, tmin):
        assert (a[:w0].view(np.uint32) == SENTINEL).all() and (a[w1:].view(np.uint32) == SENTINEL).all(), (what, "rows outside", w0, w1)
    for t in tails:
        assert (t.view(np.uint32) == SENTINEL).all(), (what, "guard tail")
    return cnt, tmin, aux


def check(key, acgt, v, cons):
    case = SE.CASES[key]
    q = engine_query(key, acgt, cons)
    assert q.ntax == case.nq
    for db_n, ranges in case.scans:
        with capi.Engine.from_query(q, nbest=5, max_pool=max(64, db_n), tuning=SE.tuning(case, v)) as eng:
            assert eng.scan_variant() == case.variant                     # no silent fallback to another scan
            assert eng.shard_rows() == (q.ntax + 127) // 128 * 128
            if case.active:
                eng.set_active_queries(*case.active)
            eng.db_reserve(db_n)
            eng.db_append(list(case.refs[:db_n]))
            for first, n in ranges:
                out = check_scan(key, acgt, q, eng, db_n, first, n)
            # 5. the rebuild of the planes derived for the query set leaves the same bytes
            eng.db_rederive()
            again = check_scan(key, acgt, q, eng, db_n, first, n)
            for a, b in zip(out, again):
                assert np.array_equal(a, b), (key, "after db_rederive")


# ---- the scans run in one worker process that loads the tensor library's runtime before the engine's (in the order a pytest process that has
# already opened engines cannot offer: tests/test_rows_gpu.py); a test sends its run and asserts on the worker's answer
_worker = None


def _stop_worker():
    global _worker
    if _worker is not None:
        try:
            _worker.stdin.close()
            _worker.wait(timeout=60)
        except Exception:
            _worker.kill()
        _worker = None


def remote_check(key, acgt, v, cons):
    global _worker
    if _worker is None:
        _worker = subprocess.Popen([sys.executable, os.path.abspath(__file__)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        atexit.register(_stop_worker)
    assert _worker.poll() is None, "the worker ended at an earlier run (an error of the engine there ends it: nothing more is started on the GPU)"
    _worker.stdin.write(json.dumps([key, acgt, v, cons]) + "\n")
    _worker.stdin.flush()
    for line in _worker.stdout:
        if line.startswith("@@"):
            answer = json.loads(line[2:])
            assert answer is None, answer
            return
    raise AssertionError("the worker ended during this run (exit status %s)" % _worker.wait())


@pytest.fixture(scope="module", autouse=True)
def _worker_ends_with_the_module():
    yield
    _stop_worker()


def worker_main():
    import traceback
    import torch
    torch.cuda.init()                                     # the tensor's runtime first, the engine's after it
    for line in sys.stdin:
        key, acgt, v, cons = json.loads(line)
        try:
            check(key, acgt, None if v is None else tuple(v), cons)
            answer = None
        except AssertionError:
            answer = traceback.format_exc()[-3000:]
        except BaseException:                             # an error of the engine or of the runtime: report it and start nothing more
            print("@@" + json.dumps("the worker stops: " + traceback.format_exc()[-3000:]), flush=True)
            return 1
        print("@@" + json.dumps(answer), flush=True)
    return 0


@cases("S")
def test_s_item_stream_of_a_group_record(key, acgt, v, cons):
    """full lists of 1, 3, 4, 5, 8 and 64 queries, 1, 2, 3 and 63 general items, word lists (1,0,0,0) (0,0,0,1) (2,0,3,0) (3,1,2,5), run items over
    one to three full words with and without a partial word, gaps and ambiguity codes, N at polymorphic columns"""
    remote_check(key, acgt, v, cons)


@cases("W")
def test_w_records_per_wave(key, acgt, v, cons):
    """3 records for 8 waves, a super-tile without records, 33 / 64 / 65 / 130 queries, the second super-tile alone (set_active_queries)"""
    remote_check(key, acgt, v, cons)


@cases("P")
def test_p_dense_polymorphic_and_rare_columns(key, acgt, v, cons):
    """0, 1, 128 and 129 dense columns; all polymorphic columns rare, none rare; rare word lists (1,0,0,0) (0,0,0,1) (2,3,1,4) over three rare groups"""
    remote_check(key, acgt, v, cons)


@cases("T")
def test_t_tiles_ranges_grid(key, acgt, v, cons):
    """1, 2, 3 and 5 tiles (dead tiles of the last wave at R = 2 and 4); ranges cut inside a tile on either side; 9 tile groups on a grid of 16 slots"""
    remote_check(key, acgt, v, cons)


@cases("C")
def test_c_counter_range(key, acgt, v, cons):
    """49 000 columns with the low half 57 below 2^16; NP4 = 126 with the low half down to 256; NP4 = 127 falls back to the packed-plane scan"""
    remote_check(key, acgt, v, cons)


@cases("K")
def test_k_packed_plane_kernels(key, acgt, v, cons):
    """QT = 1, 2, 4, 8, 16 with padding queries in the last tile, with and without the consensus pre-score, over the tile and range edges of T"""
    remote_check(key, acgt, v, cons)


@cases("S", "W", "P")
def test_the_engine_built_the_stream_the_model_describes(key, acgt, v, cons):
    """query tables 7 (item stream), 8 (shares of the waves) and 10 (counts) against scan_edges.Model: the case reaches its edge on the device too"""
    case, q = SE.CASES[key], SE.query(key, acgt)
    m = SE.model(key, acgt, v[0])
    with capi.Engine.from_query(q, nbest=5, max_pool=64, tuning=SE.tuning(case, v)) as eng:
        counts = eng.query_table(10).view(np.int32)
        stream, sdir = eng.query_table(7).view(np.uint32), eng.query_table(8).view(np.uint32)
    assert [int(x) for x in counts[:6]] == [m.NP, m.NR, m.NP4, m.NR4, m.rare_max, m.variant]
    tiles = SE.decode_stream(stream, sdir, m.n_st, v[0], v[1])
    for st, (recs, rares, shares, rshares) in enumerate(tiles):
        assert recs == m.records[st], (key, st)
        assert [(h0, r.words) for h0, r in rares] == [((m.NP4 + r.r4) * 3072, r.words) for r in m.rare_records[st]], (key, st)
        assert shares == m.record_shares(st) and rshares == m.rare_shares(st), (key, st)


if __name__ == "__main__":
    sys.exit(worker_main())
