"""Every way rows enter the resident database -- uvaia_gpu_db_append, _append_block, _append_packed, _append_device, _append_staged -- at its
refusals: a full database, a byte outside the alphabet, a context that was never reserved; and the life cycle of a context that uses
everything it allocates on first use, three times in one process, behind an open that fails half way."""
import numpy as np
import pytest

import rows_lib as R
from test_rows_gpu import DeviceBlock, _query
from uvaia_amd import capi

pytestmark = pytest.mark.gpu

NQ, NCHAR, N = 3, 200, 130            # a partial last word group; two tiles plus two lanes
WAYS = ("append", "append_block", "append_packed", "append_device", "append_staged")
ESTATE, EALPHABET = -6, -5

_rows, _tiles_of = None, {}


def rows():
    global _rows
    if _rows is None:
        _rows = R.random_rows(200, NCHAR, seed=29, special=True)
    return _rows


def engine(acgt, **kw):
    return capi.Engine.from_query(_query(NCHAR, acgt, nq=NQ), nbest=4, **{"max_pool": 64, **kw})


def tiles(first, n):
    """rows()[first:first + n] in the packed interchange form (planes, valid-site counts, side rows), as a default-mode context exports them"""
    if (first, n) not in _tiles_of:
        with engine(False) as eng:
            eng.db_append(rows()[first:first + n])
            _tiles_of[(first, n)] = eng.db_export()
    return _tiles_of[(first, n)]


def enter(eng, way, first, n, spoil=False):
    """rows()[first:first + n] into the resident database of eng through one of the five entries; spoil: the first row holds a 'J'"""
    rr = list(rows()[first:first + n])
    if spoil:
        rr[0] = rr[0][:7] + b"J" + rr[0][8:]
    if way == "append":
        eng.db_append(rr)
    elif way == "append_block":
        block = np.full((n, NCHAR + 5), ord("N"), dtype=np.uint8)
        for i, r in enumerate(rr):
            block[i, :NCHAR] = np.frombuffer(r, dtype=np.uint8)
        eng.db_append_block(block)
    elif way == "append_device":
        t = DeviceBlock(rr, NCHAR, NCHAR + 3, 1)
        eng.db_append_device(t.ptr, **t.args())
    else:
        planes, non_n, side = tiles(first, n)
        if way == "append_packed":
            eng.db_append_packed(planes, non_n, side, n)
        else:
            eng.db_stage_reserve(planes.shape[0])
            eng.db_stage_packed(0, planes, non_n, side, planes.shape[0])
            eng.db_append_staged(0, None, n)


def heaps(eng):
    eng.reset()
    eng.search_resident(64)
    return [x.copy() for x in eng.drain()]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("way", WAYS)
def test_a_refused_append_leaves_the_database_and_the_next_one_works(way, acgt):
    resident, more = (64, 128) if way == "append_packed" else (100, 64)      # (packed tiles follow a whole tile)
    with engine(acgt) as eng:
        eng.db_reserve(128)
        eng.db_append(rows()[:resident])
        before = heaps(eng)
        assert int(before[0].sum()) > 0
        with pytest.raises(capi.GpuError) as err:
            enter(eng, way, resident, more)
        assert err.value.code == ESTATE and "database capacity 128 exceeded: call uvaia_gpu_db_reserve first" in str(err.value)
        assert eng.db_size() == resident
        assert same(heaps(eng), before)
        if way in ("append", "append_device"):
            with pytest.raises(capi.GpuError) as err:
                enter(eng, way, resident, 10, spoil=True)
            assert err.value.code == EALPHABET
            assert eng.db_size() == resident
        n_good = 64 if way == "append_packed" else 10
        enter(eng, way, resident, n_good)
        assert eng.db_size() == resident + n_good
        got = heaps(eng)
    with engine(acgt) as ref:
        ref.db_reserve(128)
        ref.db_append(rows()[:resident])
        enter(ref, way, resident, n_good)
        assert same(got, heaps(ref))


@pytest.mark.parametrize("acgt", [False, True])
@pytest.mark.parametrize("way", WAYS)
def test_the_first_append_of_an_unreserved_context_reserves_for_itself(way, acgt):
    with engine(acgt) as eng:
        enter(eng, way, 0, 70)
        assert eng.db_size() == 70
        got = heaps(eng)
        assert int(got[0].sum()) > 0
        with pytest.raises(capi.GpuError) as err:
            enter(eng, way, 70, 70)
        assert err.value.code == ESTATE
        if way != "append_packed":                                           # (there the 70 resident ones are no whole number of tiles: refused for that)
            assert "database capacity 128 exceeded" in str(err.value)
        assert eng.db_size() == 70
        assert same(heaps(eng), got)
    with engine(acgt) as ref:
        ref.db_reserve(70)
        enter(ref, way, 0, 70)
        assert same(got, heaps(ref))


def _one_life(acgt, block):
    """a context that uses everything allocated on first use; what it computed"""
    rr, out = list(rows()[:N]), []
    planes, non_n, side = tiles(0, N)
    with engine(acgt, max_pool=192, tuning={"scan": "compressed"}) as eng:
        out.append(eng.push(rr))
        out.append(eng.last_batch_scores(N))
        out += eng.drain()
        eng.reset()
        eng.db_reserve(N)
        eng.db_append(rr[:64])
        eng.db_rederive()
        out.append(eng.search_resident(64))
        out += eng.drain()
        out.append(eng.ball(rr, 5))
        out.append(eng.ball_packed(planes, N, 5))
        out.append(np.frombuffer(b"".join(eng.unpack_rows([0, 129, 64])), dtype=np.uint8))
        census = eng.rows_census(block.ptr, **block.args())
        out += census
        eng.db_append_device(block.ptr, row_index=list(range(64, N)), **block.args())
        out += eng.rows_exceptions(block.ptr, census[1], **block.args())
        eng.reset()
        eng.db_rederive()
        out.append(eng.search_resident(64))
        out += eng.drain()
        eng.db_stage_reserve(planes.shape[0])
        eng.db_stage_packed(0, planes, non_n, side, planes.shape[0])
        eng.db_load_staged(0, None, N)
        out.append(np.frombuffer(b"".join(eng.db_unpack_rows([1, 129])), dtype=np.uint8))
        eng.reset()
        out.append(eng.search_resident(64))
        out += eng.drain()
        out.append(eng.agree_on_polymorphic(rr[:10]))
    return out


@pytest.mark.parametrize("acgt", [False, True])
def test_three_lives_in_one_process_behind_a_failed_open(acgt):
    q = _query(NCHAR, acgt, nq=NQ)
    spoilt = list(q.seqs)
    spoilt[NQ - 1] = spoilt[NQ - 1][:50] + b"J" + spoilt[NQ - 1][51:]
    with pytest.raises(capi.GpuError) as err:                                # the tables of two good rows and the staging buffers exist by then
        capi.Engine(spoilt, q.consensus, q.idx_c, q.idx_m, q.idx, trim=q.trim, acgt=acgt, nbest=4, max_pool=192)
    assert err.value.code == EALPHABET
    block = DeviceBlock(list(rows()[:N]), NCHAR, NCHAR + 3, 1)
    lives = [_one_life(acgt, block) for _ in range(3)]
    assert len(lives[0]) == len(lives[2]) and same(lives[0], lives[2]) and same(lives[0], lives[1])
    assert int(lives[0][2].sum()) > 0 and int(lives[0][-5].sum()) > 0      # heaps of the push and of the last resident search hold something
