"""GPU tier of the softmax queries of the exact index (clip_amd_index_softmax[_ids | _index | _device]; k_softmax.hip).  distances and ids
are compared with the search of the same name as uint32 bits / integers; probs and log_z against tests/softmax_common.py, float64 over
the complete distance list that range_search at radius 4 (or a search with k = every row) returns, which has search's bits.

Bounds (profiles/softmax_accuracy.txt): the largest errors measured on an MI355X over exactly these cases were 2.876e-7 relative for
probs and 7.629e-6 absolute for log_z (half a unit in the last place of an f32 between 128 and 256: log_z is about -scale m); each bound
is 4x its figure, the margin for v_exp_f32's last place and the f32 accumulation, which vary with shape.  A prob below f32's smallest
normal cannot carry a relative error: it is compared absolutely against that value."""
import ctypes as C

import numpy as np
import pytest

from index_subset_common import DTYPES
from softmax_common import softmax_reference

pytestmark = pytest.mark.gpu

PROB_RTOL, LOGZ_ATOL = 4 * 2.876e-7, 4 * 7.629e-6
TINY = float(np.finfo(np.float32).tiny)
ROWS = [1, 63, 65, 257]                  # 257: one row more than the smallest chunk the launcher picks (256, as rank's)
POISON = -77.0


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, searched, full, eligible, beta, n):
    """got = (distances, ids, probs, log_z) of a softmax call; searched = the search of the same name; full = (lims, dist, ids)"""
    dist, ids, probs, log_z = got
    assert np.array_equal(bits(dist), bits(searched[0])) and np.array_equal(ids, searched[1])
    want_p, want_z = softmax_reference(*full, eligible, beta, n)
    want = np.where(ids >= 0, np.take_along_axis(want_p, np.maximum(ids, 0), axis=1), 0.0)
    big = want >= TINY
    rel = float(np.max(np.abs(probs[big] - want[big]) / want[big], initial=0.0))
    some = np.isfinite(want_z)
    err_z = float(np.max(np.abs(log_z[some] - want_z[some]), initial=0.0))
    print("softmax_accuracy prob_rel %.3e log_z_abs %.3e" % (rel, err_z))
    assert rel <= PROB_RTOL and err_z <= LOGZ_ATOL
    assert np.all(np.abs(probs[~big] - want[~big]) <= TINY) and np.all(probs[ids < 0] == 0)
    assert np.all(np.isneginf(log_z[~some])) and np.all(probs[~some] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [4, 36, 512])
def test_shapes(clip, clip_lib, dtype, dim):
    rng = np.random.default_rng(7 * dim)
    for n in ROWS:
        ix = clip_lib.Index(clip, dim, dtype)
        ix.add(rng.standard_normal((n, dim), dtype=np.float32))
        for nq in (1, 17, 65):
            q = rng.standard_normal((nq, dim), dtype=np.float32)
            full = ix.range_search(q, 4.0)
            for k, beta in ((1, 100.0), (10, 1.0), (10, 100.0)):          # k = 10 exceeds the eligible rows at n = 1
                got = ix.softmax(q, k, scale=beta)
                check(got, ix.search(q, k), full, np.ones(n, dtype=bool), beta, n)
            again = ix.softmax(q, 10, scale=100.0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))      # two identical calls: identical bytes
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_eligibility(clip, clip_lib, dtype):
    import torch
    n, dim, k = 257, 36, 10
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((17, dim), dtype=np.float32)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    allow = np.ones(n, dtype=bool)
    allow[32:96] = False                                                # two whole 32-row words
    allow[[0, 5, 130, 256]] = False                                     # single rows
    ix.remove([7, 100, 255])
    live = ix.live_mask()
    for a in (None, allow):
        el = live if a is None else live & a
        check(ix.softmax(q, k, scale=100.0, allow=a), ix.search(q, k, allow=a), ix.range_search(q, 4.0, allow=a), el, 100.0, n)
    # stored rows as the queries: the complete list is search_ids with k = every row
    ids = np.array([3, 64, 64, 256, 128], dtype=np.int64)
    for ex in (True, False):
        D, I = ix.search_ids(ids, n, exclude_self=ex, allow=allow)
        full = (np.arange(len(ids) + 1) * n, D.reshape(-1), I.reshape(-1))
        el = np.tile(live & allow, (len(ids), 1))
        el[np.arange(len(ids)), ids] &= not ex
        check(ix.softmax_ids(ids, k, scale=1.0, exclude_self=ex, allow=allow), ix.search_ids(ids, k, exclude_self=ex, allow=allow), full, el, 1.0, n)
    # the rows of a second index as the queries
    src = clip_lib.Index(clip, dim, dtype)
    src.add(q)
    D, I = ix.search_index(src, n, allow=allow)
    full = (np.arange(len(q) + 1) * n, D.reshape(-1), I.reshape(-1))
    check(ix.softmax_index(src, k, scale=100.0, allow=allow), ix.search_index(src, k, allow=allow), full, live & allow, 100.0, n)
    src.close()
    # no eligible row: -inf and zeros; and the device form over poisoned buffers of one slot more: the bytes of the host form
    _, I, P, Z = ix.softmax(q, k, allow=np.zeros(n, dtype=bool))
    assert np.all(np.isneginf(Z)) and np.all(P == 0) and np.all(I == -1)
    words = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64)).cuda()
    dq = torch.from_numpy(q).cuda()
    dd, dp = (torch.full((17 * k + 1,), POISON, dtype=torch.float32, device="cuda") for _ in range(2))
    di = torch.full((17 * k + 1,), int(POISON), dtype=torch.int64, device="cuda")
    dz = torch.full((18,), POISON, dtype=torch.float32, device="cuda")
    ix.softmax_device(dq.data_ptr(), 17, k, dd.data_ptr(), di.data_ptr(), dp.data_ptr(), dz.data_ptr(), scale=100.0, d_allow=words.data_ptr())
    clip.synchronize()
    host = ix.softmax(q, k, scale=100.0, allow=allow)
    for dev, h in zip((dd, di, dp, dz), host):
        assert dev[-1].item() == POISON and np.array_equal(dev[:-1].cpu().numpy().reshape(h.shape).view(np.uint8), np.ascontiguousarray(h).view(np.uint8))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_range(clip, clip_lib, dtype):
    n, dim = 65, 36
    rng = np.random.default_rng(5)
    q = np.zeros((1, dim), dtype=np.float32)
    q[0, 0] = 1.0
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    rows[:, 0] = 0.0                                                    # every row at d = 1: sum exp(-100 d) would flush to 0
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    got = ix.softmax(q, n, scale=100.0)
    check(got, ix.search(q, n), ix.range_search(q, 4.0), np.ones(n, dtype=bool), 100.0, n)
    assert np.all(np.isfinite(got[2])) and np.isfinite(got[3][0]) and abs(float(got[2].astype(np.float64).sum()) - 1.0) <= PROB_RTOL
    ix.close()
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(np.concatenate([q, -q]))                                     # an identical row next to an antipodal one, d = 0 and 2
    got = ix.softmax(q, 2, scale=100.0)
    check(got, ix.search(q, 2), ix.range_search(q, 4.0), np.ones(2, dtype=bool), 100.0, 2)
    assert list(got[1][0]) == [0, 1] and got[2][0, 0] == 1.0 and got[2][0, 1] == 0.0
    ix.close()


def test_refusals(clip, clip_lib, capfd):
    ix = clip_lib.Index(clip, 36, "f16")
    ix.add(np.random.default_rng(3).standard_normal((65, 36), dtype=np.float32))
    q = np.ones((2, 36), dtype=np.float32)
    f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    D, P, Z = (np.full(2 * 1025, POISON, dtype=np.float32) for _ in range(3))
    I = np.full(2 * 1025, int(POISON), dtype=np.int64)
    for k, beta in ((5, 0.0), (5, float("nan")), (5, float("inf")), (5, -1.0), (0, 100.0), (1025, 100.0)):
        ok = clip_lib.lib().clip_amd_index_softmax(ix.handle, q.ctypes.data_as(f32p), 2, k, beta, None, D.ctypes.data_as(f32p), I.ctypes.data_as(i64p),
                                                   P.ctypes.data_as(f32p), Z.ctypes.data_as(f32p))
        assert ok is False and capfd.readouterr().err.strip()
        assert np.all(D == POISON) and np.all(P == POISON) and np.all(Z == POISON) and np.all(I == int(POISON))
    ix.close()
