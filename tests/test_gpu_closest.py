"""GPU tier of the closest pairs of the exact index (k_closest.hip, clip_amd_index_closest_pairs).  The oracle is the contract's own
sentence: `Index.pairs(4.0)` restricted to eligible rows and by labels, sorted by (d, lo, hi) and cut (tests/closest_common.py).  Every
comparison is for equality of bits; no tolerance appears anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from closest_common import reference
from extents_common import clustered, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("f16", "f32", "i8")
N = 333                                                                        # three row tiles, the last one partial
SHAPES = [(dtype, dim) for dim in (512, 72) for dtype in DTYPES]                # dim 72: a last chunk of fewer than 4 k-steps


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def cases(clip, clip_lib):
    """per (dtype, dim): the index of N clustered rows and its whole pair list; built once, shared by the tests, never changed"""
    built = {}

    def get(dtype, dim):
        if (dtype, dim) not in built:
            ix = clip_lib.Index(clip, dim, dtype)
            ix.add(clustered(np.random.default_rng(dim + len(dtype)), N, dim))
            pairs = ix.pairs(4.0)
            assert len(pairs[0]) == N * (N - 1) // 2
            built[(dtype, dim)] = (ix, pairs)
        return built[(dtype, dim)]
    yield get
    for ix, _ in built.values():
        ix.close()


@pytest.mark.parametrize("dtype,dim", SHAPES)
def test_result_equals_the_sorted_pair_list(cases, dtype, dim):
    ix, pairs = cases(dtype, dim)
    for n in (1, 7, 1024):
        got = ix.closest_pairs(n)
        assert len(got[0]) == n and same_bits(got, reference(n, *pairs))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_at_the_cut_and_paging(clip, clip_lib, dtype):
    rng = np.random.default_rng(3)
    n, dim = 200, 72
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    where = rng.permutation(n)
    copies, zeros = np.sort(where[:64]), where[64:80]
    rows[copies] = rows[copies[0]]                                              # 2016 pairs at one distance
    rows[zeros] = 0                                                             # at distance exactly 1 from everything
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    pairs = ix.pairs(4.0)
    tie = np.isin(pairs[0], copies) & np.isin(pairs[1], copies)
    assert tie.sum() == 2016 and len(np.unique(pairs[2][tie].view(np.uint32))) == 1 and pairs[2][tie][0] < pairs[2][~tie].min()
    assert np.all(pairs[2][np.isin(pairs[0], zeros) | np.isin(pairs[1], zeros)] == 1)
    lo, hi, d = ix.closest_pairs(100)                                           # the 100 lowest (lo, hi) of the tie
    assert same_bits((lo, hi, d), reference(100, *pairs)) and np.all(np.isin(lo, copies) & np.isin(hi, copies))
    whole = ix.closest_pairs(1024)                                              # cuts inside the tie
    assert same_bits(whole, reference(1024, *pairs))
    pages, after = [], None
    for _ in range(22):                                                         # 2200 pairs: through the tie and past it
        page = ix.closest_pairs(100, after=after)
        assert same_bits(page, reference(100, *pairs, after=after))
        after = (page[2][-1], page[0][-1], page[1][-1])
        pages.append(page)
    paged = [np.concatenate(f) for f in zip(*pages)]
    assert same_bits([f[:1024] for f in paged], whole) and same_bits(paged, reference(2200, *pairs))
    ix.close()


def test_fewer_candidates_than_asked(cases, clip_lib):
    ix, pairs = cases("f16", 72)
    allow = np.zeros(N, dtype=bool)
    allow[np.random.default_rng(4).choice(N, 40, replace=False)] = True
    want = reference(1024, *pairs, eligible=allow)
    assert len(want[0]) == 780 and same_bits(ix.closest_pairs(1024, allow=allow), want)
    d = np.full(1024, -7, dtype=np.float32)
    lo, hi = np.full(1024, -7, dtype=np.int64), np.full(1024, -7, dtype=np.int64)
    i64p, words = C.POINTER(C.c_int64), clip_lib.allow_words(allow, N)
    m = clip_lib.lib().clip_amd_index_closest_pairs(ix.handle, 1024, words.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, 0, 0,
                                                    d.ctypes.data_as(C.POINTER(C.c_float)), lo.ctypes.data_as(i64p), hi.ctypes.data_as(i64p))
    assert m == 780 and same_bits((lo[:m], hi[:m], d[:m]), want)
    assert np.all(np.isposinf(d[m:])) and np.all(lo[m:] == -1) and np.all(hi[m:] == -1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_removed_rows_and_allow_equal_a_fresh_index(clip, clip_lib, dtype):
    dim = 72
    rng = np.random.default_rng(5)
    rows = clustered(np.random.default_rng(dim + len(dtype)), N, dim)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows[:100])
    ix.add(rows[100:])                                                          # another split across add calls
    removed = rng.choice(N, 40, replace=False)
    ix.remove(removed)
    allow = rng.random(N) < 0.7
    allow[128:256] = False                                                      # a whole tile without an eligible row
    eligible = allow.copy()
    eligible[removed] = False
    keep = np.flatnonzero(eligible)
    fresh = clip_lib.Index(clip, dim, dtype)
    fresh.add(rows[keep])
    for n, use in ((50, allow), (1024, allow), (50, None)):
        lo, hi, d = ix.closest_pairs(n, allow=use)
        if use is None:                                                         # only the removed rows are out
            ids = np.setdiff1d(np.arange(N), removed)
            other = clip_lib.Index(clip, dim, dtype)
            other.add(rows[ids])
            want = other.closest_pairs(n)
            other.close()
        else:
            ids, want = keep, fresh.closest_pairs(n)
        assert same_bits((lo, hi, d), (ids[want[0]], ids[want[1]], want[2]))
    assert same_bits(fresh.closest_pairs(1024), reference(1024, *fresh.pairs(4.0)))
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_across_labels(cases, dtype):
    ix, pairs = cases(dtype, 72)
    rng = np.random.default_rng(6)
    labels = rng.integers(0, 6, N).astype(np.int64)
    labels[rng.random(N) < 0.15] = -1
    allow = rng.random(N) < 0.8
    for n in (9, 1024):
        assert same_bits(ix.closest_pairs(n, labels=labels), reference(n, *pairs, labels=labels))
        assert same_bits(ix.closest_pairs(n, labels=labels, allow=allow), reference(n, *pairs, labels=labels, eligible=allow))
    tiles = np.arange(N, dtype=np.int64) // 128 * 1000                          # whole row tiles of one label: the diagonal tiles are skipped
    tiles[300:] = 2 ** 31 - 1
    got = ix.closest_pairs(1024, labels=tiles)
    assert same_bits(got, reference(1024, *pairs, labels=tiles)) and np.all(tiles[got[0]] != tiles[got[1]])


@pytest.mark.parametrize("dtype", ("f16", "i8"))
def test_many_tiles_per_workgroup(clip, clip_lib, dtype):
    n, dim, k = 4096, 64, 16                                                    # 32 row tiles, 528 tile pairs: workgroups walk several tiles
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(clustered(np.random.default_rng(8), n, dim))
    dist, ids = ix.knn_graph(k)                                                 # every global top-16 pair lies in it, with search's bits
    row = np.repeat(np.arange(n, dtype=np.int64), k)
    up = ids.reshape(-1) > row                                                  # the orientation of pairs: the lower id is the query
    want = reference(k, row[up], ids.reshape(-1)[up], dist.reshape(-1)[up])
    got = ix.closest_pairs(k)
    assert same_bits(got, want) and same_bits(got, ix.closest_pairs(k))
    got = ix.closest_pairs(1024)                                                # a full pool carried from tile to tile
    near = ix.pairs(float(got[2][-1]))                                          # every pair up to the last distance returned, ties included
    assert same_bits(got, reference(1024, *near)) and same_bits(got, ix.closest_pairs(1024))
    ix.close()


def test_device_form_save_load_and_refusals(clip, clip_lib, cases, tmp_path, capfd):
    import torch
    ix, pairs = cases("i8", 72)
    rng = np.random.default_rng(13)
    labels = rng.integers(-1, 5, N).astype(np.int64)
    allow = rng.random(N) < 0.8
    after = (pairs[2][40], int(pairs[0][40]), int(pairs[1][40]))
    first = ix.closest_pairs(300, allow=allow, labels=labels, after=after)
    assert same_bits(first, reference(300, *pairs, eligible=allow, labels=labels, after=after))
    p = str(tmp_path / "rows.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert same_bits(first, loaded.closest_pairs(300, allow=allow, labels=labels, after=after))
    loaded.close()
    tl = torch.from_numpy(labels).cuda()
    tw = torch.from_numpy(clip_lib.allow_words(allow, N).view(np.int64).copy()).cuda()
    lo, hi = (torch.full((300,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    d = torch.full((300,), -7, dtype=torch.float32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.closest_pairs_device(300, lo, hi, d, count, d_allow=tw, d_labels=tl, after=after)
    clip.synchronize()
    m = int(count.item())
    assert m == len(first[0]) == 300 and same_bits((lo.cpu().numpy(), hi.cpu().numpy(), d.cpu().numpy()), first)

    L = clip_lib.lib()
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    hd, hlo, hhi = np.full(8, -7, dtype=np.float32), np.full(8, -7, dtype=np.int64), np.full(8, -7, dtype=np.int64)
    out = (hd.ctypes.data_as(f32p), hlo.ctypes.data_as(i64p), hhi.ctypes.data_as(i64p))
    at = lambda v: C.byref(C.c_float(v))
    capfd.readouterr()
    assert L.clip_amd_index_closest_pairs(None, 8, None, None, None, 0, 0, *out) == -1
    for missing in range(3):
        assert L.clip_amd_index_closest_pairs(ix.handle, 8, None, None, None, 0, 0, *[None if i == missing else o for i, o in enumerate(out)]) == -1
    for n in (0, -1, 1025):
        assert L.clip_amd_index_closest_pairs(ix.handle, n, None, None, None, 0, 0, *out) == -1
    for bad in ((float("nan"), 0, 1), (0.5, 5, 5), (0.5, 6, 5), (0.5, -1, 5), (0.5, 5, N)):
        assert L.clip_amd_index_closest_pairs(ix.handle, 8, None, None, at(bad[0]), bad[1], bad[2], *out) == -1
    assert L.clip_amd_index_closest_pairs_device(ix.handle, 1025, None, None, None, 0, 0, d.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                 count.data_ptr()) is False
    assert L.clip_amd_index_closest_pairs_device(ix.handle, 8, None, None, None, 0, 0, d.data_ptr(), lo.data_ptr(), None, count.data_ptr()) is False
    assert "n_pairs = 1025 outside 1 ... 1024" in capfd.readouterr().err
    assert np.all(hd == -7) and np.all(hlo == -7) and np.all(hhi == -7)
    assert same_bits((lo.cpu().numpy(), hi.cpu().numpy(), d.cpu().numpy()), first)      # the device outputs too
    with pytest.raises(ValueError):
        ix.closest_pairs(0)
    with pytest.raises(ValueError):
        ix.closest_pairs(5, after=(0.5, 7, 7))
    empty = clip_lib.Index(clip, 72, "f16")
    assert L.clip_amd_index_closest_pairs(empty.handle, 8, None, None, None, 0, 0, *out) == 0
    assert np.all(np.isposinf(hd)) and np.all(hlo == -1) and np.all(hhi == -1) and all(a.size == 0 for a in empty.closest_pairs(8))
    empty.close()


# ---- image_search closest ----

def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def test_image_search_closest(tmp_path, fixture_cache, clip_lib):
    from PIL import Image
    from oracle import fixtures
    rng = np.random.default_rng(12)
    imgs = tmp_path / "pictures"
    for i in range(48):                                                         # four folders of twelve: 1128 pairs, more than one page
        os.makedirs(imgs / ("f%d" % (i % 4)), exist_ok=True)
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 48)), int(rng.integers(24, 48)), 3), dtype=np.uint8)
        Image.fromarray(arr).save(imgs / ("f%d" % (i % 4)) / ("img%d.png" % i), format="PNG")
    model, db = fixtures.cached_model(fixture_cache, "tiny", "f32"), tmp_path / "db"
    r = run("build", "-m", model, "-v", "0", "--dtype", "f32", "--db", db, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (db / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 48
    clip = clip_lib.Clip(model, verbosity=0)
    index = clip_lib.Index.load(clip, str(db / "images.index"))
    every = reference(1500, *index.pairs(4.0))
    folders = np.unique([os.path.dirname(p) for p in paths], return_inverse=True)[1].astype(np.int64)
    across = index.closest_pairs(20, labels=folders)
    inside = index.closest_pairs(5, allow=np.array([p.startswith(str(imgs / "f1")) for p in paths]))
    assert same_bits(index.closest_pairs(1024), [f[:1024] for f in every]) and len(every[0]) == 1128
    index.close()
    clip.close()
    lines = lambda res: ["%f\t%s\t%s" % (d, paths[a], paths[b]) for a, b, d in zip(*res)]
    for argv, want in ((("-n", 1500), every), (("-n", 20, "--across"), across), (("-n", 5, "--in", imgs / "f1"), inside)):
        r = run("closest", "--db", db, *argv)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out = r.stdout.splitlines()
        assert out[out.index("closest:") + 1:] == lines(want) + ["main: %d pairs" % len(want[0])]
    assert all(os.path.dirname(paths[a]) != os.path.dirname(paths[b]) for a, b in zip(across[0], across[1])) and len(across[0]) == 20
    (db / "images.regions").write_text("grid 2\n")
    r = run("closest", "--db", db)
    assert r.returncode == 1 and "`closest` does not support such a database yet" in r.stderr
