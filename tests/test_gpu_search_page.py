"""GPU tier of selection at any depth (clip_amd_index_select / _search_page, k_select.hip).  The reference is the index's own exhaustive
route: range_search(queries, 4.0, allow) lists every eligible row with search's bits, a host lexsort by (distance, id) makes the full
ranking.  Distances are compared as uint32 bits and ids as integers: no tolerance anywhere.  The galleries put page boundaries inside
tie runs: every distinct vector 40 times, interleaved; or 600 of 1000 rows zero (distance exactly 1 to everything), across an id digit."""
import ctypes as C

import numpy as np
import pytest

from index_subset_common import DTYPES, open_clip

pytestmark = pytest.mark.gpu

# (rows, dim, queries): one partial chunk with padded rows; several chunks, ids past 256, three query blocks of two ranks; deeper than a page
SHAPES = [(70, 36, 1), (1000, 64, 65), (1500, 512, 17)]
WAYS = ["all", "removed", "allow"]
POISON = -77


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def made(clip_lib, fixture_cache):
    """made(dtype, shape, way) -> (index, queries, allow, ranking): ranking[i] = (distances, ids) of query i over every eligible row,
    from range_search and a host sort; built once per case and shared"""
    clip = open_clip(clip_lib, fixture_cache)
    cache = {}

    def make(dtype, shape, way):
        if (dtype, shape, way) not in cache:
            n, dim, nq = shape
            rng = np.random.default_rng(n + dim)
            if n == 1000:
                rows = rng.standard_normal((n, dim), dtype=np.float32)
                rows[rng.random(n) < 0.6] = 0.0
            else:
                rows = rng.standard_normal((-(-n // 40), dim), dtype=np.float32)[np.arange(n) % -(-n // 40)]
            q = rng.standard_normal((nq, dim), dtype=np.float32)
            q[0] = rows[np.flatnonzero(rows.any(axis=1))[0]]                # an exact match: distances at and below 0
            ix = clip_lib.Index(clip, dim, dtype)
            ix.add(rows)
            pick = rng.random(n) < 0.3
            if way == "removed":
                ix.remove(np.flatnonzero(pick))
            allow = ~pick if way == "allow" else None
            lims, d, i = ix.range_search(q, 4.0, allow=allow)
            ranking = []
            for a, b in zip(lims[:-1], lims[1:]):
                o = np.lexsort((i[a:b], d[a:b]))
                ranking.append((d[a:b][o], i[a:b][o]))
            assert all(len(r[1]) == (n if way == "all" else n - pick.sum()) for r in ranking)
            cache[(dtype, shape, way)] = (ix, q, allow, ranking)
        return cache[(dtype, shape, way)]

    make.clip = clip
    yield make
    for ix, _, _, _ in cache.values():
        ix.close()
    clip.close()


def expect(ranking, offset, k):
    """places offset ... offset + k - 1 of every query's ranking, +inf / -1 past its end"""
    d = np.full((len(ranking), k), np.inf, dtype=np.float32)
    i = np.full((len(ranking), k), -1, dtype=np.int64)
    for r, (rd, ri) in enumerate(ranking):
        m = len(ri[offset:offset + k])
        d[r, :m], i[r, :m] = rd[offset:offset + k], ri[offset:offset + k]
    return d, i


def same(got, want):
    return np.array_equal(np.asarray(got[1]), want[1]) and np.array_equal(bits(got[0]), bits(want[0]))


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_page(made, dtype, shape, way):
    ix, q, allow, ranking = made(dtype, shape, way)
    E = len(ranking[0][1])
    for k in (1, 10, 1024):
        for offset in (0, 1, 1023, 1024, E - 5, E, E + 100):
            assert same(ix.search_page(q, k, offset=offset, allow=allow), expect(ranking, offset, k)), (k, offset)
        assert same(ix.search_page(q, k, allow=allow), ix.search(q, k, allow=allow))
    pages = [ix.search_page(q, 64, offset=o, allow=allow) for o in range(0, E + 64, 64)]
    whole = np.concatenate([p[0] for p in pages], axis=1), np.concatenate([p[1] for p in pages], axis=1)
    assert same(whole, expect(ranking, 0, whole[1].shape[1])) and np.all(np.sort(whole[1][:, :E], axis=1) == np.sort(ranking[0][1]))


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_select(made, dtype, shape, way):
    ix, q, allow, ranking = made(dtype, shape, way)
    E = len(ranking[0][1])
    ranks = [0, 1, 255, 256, E - 1, E]
    for r in ranks:
        want = expect(ranking, r, 1)
        got = ix.select(q, r, allow=allow)
        assert same((got[0][:, None], got[1][:, None]), want) and same(ix.search_page(q, 1, offset=r, allow=allow), want), r
    per = np.resize(np.array(ranks, dtype=np.int64), len(q))               # one rank per query
    got = ix.select(q, per, allow=allow)
    want = [expect(ranking[i:i + 1], int(r), 1) for i, r in enumerate(per)]
    assert same(got, (np.concatenate([w[0][0] for w in want]), np.concatenate([w[1][0] for w in want])))


def test_device_forms(made, clip_lib):
    import torch
    ix, q, allow, ranking = made("f16", SHAPES[1], "allow")
    nq, k, offset = len(q), 10, 300
    dq = torch.from_numpy(q).cuda()
    words = torch.from_numpy(clip_lib.allow_words(allow, len(allow)).view(np.int64)).cuda()
    ranks = torch.arange(nq, dtype=torch.int64, device="cuda") * 9
    dd, di = torch.full((nq * k + 1,), float(POISON), device="cuda"), torch.full((nq * k + 1,), POISON, dtype=torch.int64, device="cuda")
    sd, si = torch.full((nq + 1,), float(POISON), device="cuda"), torch.full((nq + 1,), POISON, dtype=torch.int64, device="cuda")
    ix.search_page_device(dq.data_ptr(), nq, k, dd.data_ptr(), di.data_ptr(), offset=offset, d_allow=words.data_ptr())
    ix.select_device(dq.data_ptr(), nq, ranks.data_ptr(), sd.data_ptr(), si.data_ptr(), d_allow=words.data_ptr())
    torch.cuda.synchronize()
    assert dd[-1].item() == POISON and di[-1].item() == POISON and sd[-1].item() == POISON and si[-1].item() == POISON
    assert same((dd[:-1].cpu().numpy().reshape(nq, k), di[:-1].cpu().numpy().reshape(nq, k)), expect(ranking, offset, k))
    assert same((sd[:-1].cpu().numpy(), si[:-1].cpu().numpy()), ix.select(q, ranks.cpu().numpy(), allow=allow))


def test_refused_arguments(made, clip_lib, capfd):
    ix, q, _, _ = made("f16", SHAPES[0], "all")
    L, f32p, i64p = clip_lib.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    dist, ids = np.full(1024, float(POISON), dtype=np.float32), np.full(1024, POISON, dtype=np.int64)
    qp, dp, ip = q.ctypes.data_as(f32p), dist.ctypes.data_as(f32p), ids.ctypes.data_as(i64p)
    bad, good = np.array([-1], dtype=np.int64), np.array([0], dtype=np.int64)
    for call in (lambda: L.clip_amd_index_select(None, qp, 1, good.ctypes.data_as(i64p), None, dp, ip),
                 lambda: L.clip_amd_index_select(ix.handle, qp, 1, bad.ctypes.data_as(i64p), None, dp, ip),
                 lambda: L.clip_amd_index_select(ix.handle, qp, 1, None, None, dp, ip),
                 lambda: L.clip_amd_index_select(ix.handle, qp, -1, good.ctypes.data_as(i64p), None, dp, ip),
                 lambda: L.clip_amd_index_search_page(None, qp, 1, 0, 5, None, dp, ip),
                 lambda: L.clip_amd_index_search_page(ix.handle, qp, 1, -1, 5, None, dp, ip),
                 lambda: L.clip_amd_index_search_page(ix.handle, qp, 1, 0, 0, None, dp, ip),
                 lambda: L.clip_amd_index_search_page(ix.handle, qp, 1, 0, 1025, None, dp, ip),
                 lambda: L.clip_amd_index_search_page(ix.handle, None, 1, 0, 5, None, dp, ip),
                 lambda: L.clip_amd_index_search_page_device(ix.handle, None, 1, -3, 5, None, None, None)):
        assert call() is False and capfd.readouterr().err.strip() and np.all(ids == POISON) and np.all(dist == POISON)
    with pytest.raises(ValueError):
        ix.select(q, -1)
    empty = clip_lib.Index(made.clip, 36, "f16")                           # an empty index answers: nothing stands anywhere
    assert same(empty.search_page(q, 3, offset=2), expect([((), ())], 0, 3)) and same(empty.select(q, 0), (np.array([np.inf]), np.array([-1])))
    empty.close()
