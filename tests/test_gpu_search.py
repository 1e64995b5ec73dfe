"""GPU tier of the exact nearest-neighbour index (k_search.hip, clip_amd_index_*): results against a float64 numpy search over the very
values the index stores (read back from a saved index file), tie order and edge cases, the device-pointer forms, bit-identity across
query / row splits and save / load, malformed files and bad arguments, and a 1 M-row gallery."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NP_DT = {"f16": np.float16, "f32": np.float32}


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def stored_rows(index, tmp_path, name="rows.index"):
    """what the index stores, unpadded, from its own file"""
    p = str(tmp_path / name)
    index.save(p)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    return np.memmap(p, dtype=np.float16 if dt == 1 else np.float32, mode="r", offset=28, shape=(n, dim))


def stored_queries(q, dtype):
    """the queries as search_normalize_kernel stores them: the f32 sum of squares in the kernel's own order (lane i % 64 adds its values in
    ascending i, then the xor butterfly 32 ... 1 over the 64 lanes), x / sqrt(ss) in f32, rounded to the stored dtype.  Any other
    summation order gives another f32 norm now and then, which flips the fp16 rounding of a value: at a small dim, where the values are
    large, one flip moves a distance by more than check's tolerance (seen with numpy's own sum: dim 36, 2 of 37080 values, 3.9e-5)."""
    q = np.asarray(q, dtype=np.float32)
    m, dim = q.shape
    sq = np.zeros((m, (dim + 63) // 64 * 64), dtype=np.float32)
    sq[:, :dim] = q * q
    lanes = np.zeros((m, 64), dtype=np.float32)
    for c in range(0, sq.shape[1], 64):
        lanes = lanes + sq[:, c:c + 64]
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ off]
    ss = lanes[:, :1]
    qn = np.where(ss > 0, q / np.where(ss > 0, np.sqrt(ss), 1), 0).astype(np.float32)
    return qn.astype(NP_DT[dtype]).astype(np.float64)


def ref_distances(rows, q64, block=131072):
    n = rows.shape[0]
    out = np.empty((q64.shape[0], n), dtype=np.float64)
    for r0 in range(0, n, block):
        out[:, r0:r0 + block] = 1.0 - q64 @ np.asarray(rows[r0:r0 + block], dtype=np.float64).T
    return out


def check(dist, ids, refd, k, dim):
    """distances within tol of the float64 reference; ids = the exact top-k except among entries within tol of the k-th; sorted, tie rule"""
    tol = dim * 2.0 ** -24 + 1e-6
    nq, n = refd.shape
    kk = min(k, n)
    assert dist.shape == (nq, k) and ids.shape == (nq, k)
    assert np.all(ids[:, kk:] == -1) and np.all(np.isinf(dist[:, kk:])) and np.all(dist[:, kk:] > 0)
    for i in range(nq):
        d, g = dist[i, :kk].astype(np.float64), ids[i, :kk]
        assert np.all((g >= 0) & (g < n)) and len(set(g.tolist())) == kk
        assert np.all(np.abs(d - refd[i, g]) <= tol), np.abs(d - refd[i, g]).max()
        assert np.all(np.diff(d) >= 0)
        same = np.diff(d) == 0
        assert np.all(np.diff(g)[same] > 0), "equal distances must come lower id first"
        top = np.argpartition(refd[i], kk - 1)[:kk] if kk < n else np.arange(n)
        kth = refd[i, top].max()
        want = set(top.tolist())
        for x in set(g.tolist()) ^ want:
            assert abs(refd[i, x] - kth) <= tol, (i, x, refd[i, x], kth)
        np.testing.assert_allclose(d, np.sort(refd[i, top]), atol=tol, rtol=0)


CASES = [  # dtype, dim, N, nq, k
    ("f16", 32, 1, 1, 1), ("f32", 32, 1, 5, 5), ("f16", 32, 7, 5, 5), ("f32", 32, 7, 64, 100), ("f16", 512, 7, 1, 1024),
    ("f16", 512, 1000, 64, 100), ("f32", 512, 1000, 5, 1024), ("f16", 768, 1000, 300, 5), ("f32", 1280, 1000, 1, 1),
    ("f16", 1024, 65537, 5, 100), ("f32", 768, 65537, 64, 5), ("f16", 1280, 65537, 1, 1024), ("f16", 512, 65537, 300, 1),
    ("f32", 1024, 65537, 5, 1024), ("f16", 512, 300000, 5, 100), ("f32", 512, 300000, 1, 5), ("f16", 768, 300000, 64, 1024),
    ("f16", 36, 300, 1030, 3), ("f32", 36, 300, 1030, 3),      # two passes over the query chunks, workspaces reused
    # k = 100 over three chunks of 448 rows: every buffer is shrunk in the middle of its chunk; 1, 2 and 4 query tiles
    ("f16", 36, 1030, 1, 100), ("f16", 36, 1030, 17, 100), ("f16", 36, 1030, 64, 100), ("f16", 512, 1030, 1, 100), ("f16", 512, 1030, 17, 100),
    ("f16", 512, 1030, 64, 100), ("f32", 36, 1030, 1, 100), ("f32", 36, 1030, 17, 100), ("f32", 36, 1030, 64, 100), ("f32", 512, 1030, 1, 100),
    ("f32", 512, 1030, 17, 100), ("f32", 512, 1030, 64, 100),
]


@pytest.mark.parametrize("dtype, dim, n, nq, k", CASES)
def test_exact_against_numpy(clip, clip_lib, tmp_path, dtype, dim, n, nq, k):
    rng = np.random.default_rng(dim * 7 + n + nq + k)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    if n > 3:
        q[0] = rows[n // 2] * 3.0                   # a query that is (a multiple of) a stored row
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    assert len(ix) == n
    dist, ids = ix.search(q, k)
    refd = ref_distances(stored_rows(ix, tmp_path), stored_queries(q, dtype))
    check(dist, ids, refd, k, dim)
    if n > 3:
        assert ids[0, 0] == n // 2 and dist[0, 0] < 1e-3 * (4 if dtype == "f16" else 1)
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_ties_tail_and_zero_vectors(clip, clip_lib, dtype):
    rng = np.random.default_rng(5)
    dim = 64
    rows = rng.standard_normal((3000, dim), dtype=np.float32)
    dup = rows[10].copy()
    dup_ids = [10, 11, 700, 1999, 2000, 2950]
    for i in dup_ids:
        rows[i] = dup
    rows[500] = 0.0
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows[:1234])
    ix.add(rows[1234:])
    d, g = ix.search(dup[None], 8)
    assert g[0, :6].tolist() == dup_ids and np.all(d[0, :6] == d[0, 0])
    z = np.zeros((2, dim), dtype=np.float32)
    d, g = ix.search(z, 5)                         # zero query: distance exactly 1 to everything, lowest ids first
    assert np.all(d == 1.0) and g.tolist() == [[0, 1, 2, 3, 4]] * 2
    zr = clip_lib.Index(clip, dim, dtype)          # zero row: distance exactly 1 to any query
    zr.add(rows[:600])
    d, g = zr.search(rng.standard_normal((4, dim), dtype=np.float32), 1024)
    assert np.all((g == 500).sum(1) == 1) and np.all(d[g == 500] == 1.0) and np.all(g[:, 600:] == -1)
    zr.close()
    small = clip_lib.Index(clip, dim, dtype)
    small.add(rows[:3])
    d, g = small.search(rows[:2], 10)
    assert np.all(g[:, 3:] == -1) and np.all(d[:, 3:] == np.inf) and sorted(g[0, :3].tolist()) == [0, 1, 2]
    empty = clip_lib.Index(clip, dim, dtype)
    d, g = empty.search(rows[:2], 3)
    assert np.all(g == -1) and np.all(d == np.inf)
    for x in (ix, small, empty):
        x.close()


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_device_forms_match_host_forms(clip, clip_lib, dtype):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    rng = np.random.default_rng(9)
    dim, n, nq, k = 512, 20000, 37, 50
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    host = clip_lib.Index(clip, dim, dtype)
    host.add(rows)
    hd, hi = host.search(q, k)
    dev = clip_lib.Index(clip, dim, dtype)
    tr, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(q).cuda()
    td = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dev.add_device(tr.data_ptr(), 7000)
    dev.add_device(tr[7000:].data_ptr(), n - 7000)
    dev.search_device(tq.data_ptr(), nq, k, td.data_ptr(), ti.data_ptr())
    clip.synchronize()
    assert len(dev) == n
    assert np.array_equal(td.cpu().numpy().view(np.uint32), hd.view(np.uint32)) and np.array_equal(ti.cpu().numpy(), hi)
    host.close()
    dev.close()


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_bit_identity_across_splits_and_save_load(clip, clip_lib, tmp_path, dtype):
    rng = np.random.default_rng(21)
    dim, n, nq, k = 768, 50000, 300, 100
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    a = clip_lib.Index(clip, dim, dtype)
    a.add(rows)
    d1, i1 = a.search(q, k)
    d2, i2 = a.search(q, k)
    assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32)) and np.array_equal(i1, i2)
    parts = [a.search(q[s], k) for s in (slice(0, 17), slice(17, 200), slice(200, 300))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]).view(np.uint32), d1.view(np.uint32))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), i1)
    b = clip_lib.Index(clip, dim, dtype)
    cuts = [0, 1, 4097, 4100, 31000, n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b.add(rows[lo:hi])
        b.search(q[:3], 7)                         # interleaved searches do not disturb later results
    d3, i3 = b.search(q, k)
    assert np.array_equal(d3.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i3, i1)
    p1, p2 = str(tmp_path / "a.index"), str(tmp_path / "b.index")
    a.save(p1)
    c = clip_lib.Index.load(clip, p1)
    assert len(c) == n and c.dim == dim
    d4, i4 = c.search(q, k)
    assert np.array_equal(d4.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i4, i1)
    c.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    b.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    for x in (a, b, c):
        x.close()


def test_malformed_files_and_bad_arguments(clip, clip_lib, tmp_path, capfd):
    L = clip_lib.lib()
    rng = np.random.default_rng(3)
    dim = 32
    ix = clip_lib.Index(clip, dim, "f16")
    ix.add(rng.standard_normal((10, dim), dtype=np.float32))
    good = str(tmp_path / "good.index")
    ix.save(good)
    raw = open(good, "rb").read()
    assert len(raw) == 28 + 10 * dim * 2

    def bad(name, data, msg):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        assert not L.clip_amd_index_load(clip.ctx, p.encode())
        assert msg in capfd.readouterr().err

    hdr = lambda ver=1, d=dim, dt=1, n=10: b"CLIPIDX1" + struct.pack("<IIIQ", ver, d, dt, n)
    bad("trunc.index", raw[:-3], "its header says")
    bad("short.index", raw[:20], "shorter than the header")
    bad("magic.index", b"CLIPIDX2" + raw[8:], "bad magic")
    bad("version.index", hdr(ver=2) + raw[28:], "version 2")
    bad("overflow.index", hdr(n=(1 << 62)) + raw[28:], "overflow")
    bad("dim.index", hdr(d=30) + raw[28:], "dim 30")
    bad("dim0.index", hdr(d=0) + raw[28:], "dim 0")
    bad("dimbig.index", hdr(d=8192) + raw[28:], "dim 8192")
    bad("dtype.index", hdr(dt=7) + raw[28:], "dtype 7")
    bad("size.index", hdr(d=64, n=10) + raw[28:], "its header says")      # dim disagrees with the payload
    assert not L.clip_amd_index_load(clip.ctx, str(tmp_path / "missing.index").encode())
    # still working after all of that
    ok = clip_lib.Index.load(clip, good)
    d0, i0 = ix.search(np.ones((1, dim), np.float32), 3)
    d1, i1 = ok.search(np.ones((1, dim), np.float32), 3)
    assert np.array_equal(d0, d1) and np.array_equal(i0, i1)

    for d, dt in ((0, 1), (3, 1), (30, 1), (4100, 1), (8192, 0), (32, 2), (32, -1)):
        assert not L.clip_amd_index_create(clip.ctx, d, dt)
    q = np.ones((2, dim), np.float32)
    dist = np.empty((2, 1025), np.float32)
    ids = np.empty((2, 1025), np.int64)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = ids.ctypes.data_as(C.POINTER(C.c_int64))
    h = ix.handle
    assert not L.clip_amd_index_search(h, fp(q), 2, 0, fp(dist), ip)
    assert not L.clip_amd_index_search(h, fp(q), 2, 1025, fp(dist), ip)
    assert not L.clip_amd_index_search(h, fp(q), -1, 5, fp(dist), ip)
    assert not L.clip_amd_index_search(h, None, 2, 5, fp(dist), ip)
    assert not L.clip_amd_index_search(h, fp(q), 2, 5, None, ip)
    assert not L.clip_amd_index_search(h, fp(q), 2, 5, fp(dist), None)
    assert not L.clip_amd_index_search_device(h, None, 2, 5, None, None)
    assert not L.clip_amd_index_search_device(h, 1, 2, 0, 1, 1)
    assert not L.clip_amd_index_add(h, None, 3)
    assert not L.clip_amd_index_add(h, fp(q), -1)
    assert not L.clip_amd_index_add_device(h, None, 3)
    assert not L.clip_amd_index_add_device(h, 1, (1 << 31))
    assert L.clip_amd_index_search(h, fp(q), 0, 5, fp(dist), ip)       # nothing to do is not an error
    assert len(ix) == 10
    with pytest.raises(ValueError):
        ix.search(np.ones((2, dim + 1), np.float32), 3)
    with pytest.raises(ValueError):
        clip_lib.Index(clip, dim, "bf16")
    ok.close()
    ix.close()


def test_one_million_rows(clip, clip_lib, tmp_path):
    torch = pytest.importorskip("torch")
    dim, n, nq, k = 512, 1 << 20, 64, 100
    ix = clip_lib.Index(clip, dim, "f16")
    g = torch.Generator(device="cuda").manual_seed(11)
    piece = 1 << 18
    for r0 in range(0, n, piece):
        t = torch.randn((piece, dim), generator=g, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        ix.add_device(t.data_ptr(), piece)
        clip.synchronize()
        del t
    q = torch.randn((nq, dim), generator=g, device="cuda", dtype=torch.float32).cpu().numpy()
    dist, ids = ix.search(q, k)
    rows = stored_rows(ix, tmp_path, "big.index")
    sub = np.array([0, 17, 40, 63])
    refd = ref_distances(rows, stored_queries(q[sub], "f16"))
    check(dist[sub], ids[sub], refd, k, dim)
    ix.close()
    os.remove(str(tmp_path / "big.index"))
