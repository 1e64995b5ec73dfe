"""GPU tier of the int8 storage mode of the exact nearest-neighbour index (Index dtype "i8", code 3; k_search.hip search_quantize_kernel and
search_scan_kernel<int8_t>): the stored bytes against a numpy restatement of the quantisation, results against a float64 numpy search over
the stored integer vectors, exact integer data through the i8 MFMA lane map, ties / tail / zero and non-finite vectors, the device-pointer
forms, bit-identity across query / row splits and save / load, malformed i8 files, recall against the f32 index, and a 1 M-row gallery."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I8 = 3


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def quantize(x):
    """the i8 mapping of include/clip_amd.h in numpy: rint((x / max|x|) * 127) in f32, the zero vector for amax 0 or any NaN / inf"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        amax = np.abs(x).max(1, keepdims=True)
        bad = ~np.isfinite(x).all(1, keepdims=True) | ~(amax > 0)
        amax = np.where(bad, np.float32(1), amax).astype(np.float32)
        q = np.rint((x / amax).astype(np.float32) * np.float32(127))
    return np.where(bad, 0, q).astype(np.int8)


def stored_rows(index, tmp_path, name="rows.index"):
    """the int8 rows the index stores, from its own file"""
    p = str(tmp_path / name)
    index.save(p)
    ver, dim, dt, n = struct.unpack("<IIIQ", open(p, "rb").read(28)[8:])
    assert dt == I8 and os.path.getsize(p) == 28 + n * dim
    return np.memmap(p, dtype=np.int8, mode="r", offset=28, shape=(n, dim))


def unit64(v):
    v = np.asarray(v, dtype=np.float64)
    nrm = np.sqrt((v * v).sum(1))[:, None]
    return np.where(nrm > 0, v / np.where(nrm > 0, nrm, 1), 0)


def ref_distances(rows, q8, block=131072):
    """float64 cosine distances of the integer vectors (zero vectors: 1)"""
    qn = unit64(q8)
    n = rows.shape[0]
    out = np.empty((qn.shape[0], n), dtype=np.float64)
    for r0 in range(0, n, block):
        out[:, r0:r0 + block] = 1.0 - qn @ unit64(rows[r0:r0 + block]).T
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


CASES = [  # dim, N, nq, k
    (32, 1, 1, 1), (32, 7, 5, 5), (100, 7, 64, 100), (512, 7, 1, 1024), (100, 1000, 64, 100), (512, 1000, 300, 5), (1280, 1000, 1, 1),
    (768, 65537, 5, 100), (1280, 65537, 1, 1024), (1024, 65537, 64, 5), (512, 300000, 5, 100), (768, 300000, 1, 1024),
    (36, 300, 1030, 3),      # two passes over the query chunks, workspaces reused
    # k = 100 over three chunks of 448 rows: every buffer is shrunk in the middle of its chunk; 1, 2 and 4 query tiles
    (36, 1030, 1, 100), (36, 1030, 17, 100), (36, 1030, 64, 100), (512, 1030, 1, 100), (512, 1030, 17, 100), (512, 1030, 64, 100),
]


@pytest.mark.parametrize("dim, n, nq, k", CASES)
def test_exact_against_numpy(clip, clip_lib, tmp_path, dim, n, nq, k):
    rng = np.random.default_rng(dim * 7 + n + nq + k)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    if n > 3:
        q[0] = rows[n // 2] * 3.0                   # a query that is (a multiple of) a stored row
    ix = clip_lib.Index(clip, dim, "i8")
    ix.add(rows)
    assert len(ix) == n
    dist, ids = ix.search(q, k)
    stored = stored_rows(ix, tmp_path)
    assert np.array_equal(stored, quantize(rows)), "stored bytes differ from the numpy quantisation"
    check(dist, ids, ref_distances(stored, quantize(q)), k, dim)
    if n > 3:
        assert ids[0, 0] == n // 2 and dist[0, 0] <= 1e-6
    ix.close()


def test_integer_data_is_stored_and_scored_exactly(clip, clip_lib, tmp_path):
    """integers in [-127, 127] with a +-127 entry quantise to themselves, so every dot is a known int32: asymmetric data through the
    MFMA lane map, the whole ranking checked against the f32 restatement of the distance formula"""
    rng = np.random.default_rng(77)
    dim, n, nq = 320, 777, 40
    rows = rng.integers(-127, 128, size=(n, dim)).astype(np.float32)
    q = rng.integers(-127, 128, size=(nq, dim)).astype(np.float32)
    rows[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-127.0, 127.0], n)
    q[np.arange(nq), rng.integers(0, dim, nq)] = rng.choice([-127.0, 127.0], nq)
    rows[5] = np.arange(dim) % 255 - 127                      # a ramp: every k position carries a different value
    q[3] = (np.arange(dim) * 7) % 255 - 127
    ix = clip_lib.Index(clip, dim, "i8")
    ix.add(rows)
    stored = np.asarray(stored_rows(ix, tmp_path))
    assert np.array_equal(stored, rows.astype(np.int8)) and np.array_equal(quantize(q), q.astype(np.int8))
    dist, ids = ix.search(q, n)
    dot = q.astype(np.int64) @ rows.astype(np.int64).T
    inv = lambda v: (np.float32(1) / np.sqrt((v.astype(np.int64) ** 2).sum(1).astype(np.float32))).astype(np.float32)
    emu = (np.float32(1) - dot.astype(np.float32) * inv(q)[:, None] * inv(rows)[None, :]).astype(np.float32)
    want = 1.0 - (dot / np.sqrt((q.astype(np.float64) ** 2).sum(1))[:, None] / np.sqrt((rows.astype(np.float64) ** 2).sum(1))[None, :])
    for i in range(nq):
        g = ids[i]
        assert sorted(g.tolist()) == list(range(n))
        np.testing.assert_allclose(dist[i], emu[i, g], atol=3e-7, rtol=0)
        np.testing.assert_allclose(dist[i], want[i, g], atol=1e-6, rtol=0)
        order = np.lexsort((np.arange(n), want[i]))
        gap = np.abs(want[i, g] - want[i, order])
        assert np.all((g == order) | (gap <= 1e-6))
    ix.close()


def test_ties_tail_zero_and_non_finite_vectors(clip, clip_lib):
    rng = np.random.default_rng(5)
    dim = 64
    rows = rng.standard_normal((3000, dim), dtype=np.float32)
    dup = rows[10].copy()
    dup_ids = [10, 11, 700, 1999, 2000, 2950]
    for i in dup_ids:
        rows[i] = dup
    rows[700] = dup * 0.5                      # a scaled copy quantises to the same bytes
    rows[500] = 0.0
    rows[501, 7] = np.nan
    rows[502, 0] = np.inf
    rows[503, 63] = -np.inf
    ix = clip_lib.Index(clip, dim, "i8")
    ix.add(rows[:1234])
    ix.add(rows[1234:])
    d, g = ix.search(dup[None], 8)
    assert g[0, :6].tolist() == dup_ids and np.all(d[0, :6] == d[0, 0]) and d[0, 0] <= 1e-6
    d, g = ix.search(2.0 * rows[1500][None], 3)           # 2x a stored row finds it first
    assert g[0, 0] == 1500 and d[0, 0] <= 1e-6
    z = np.zeros((2, dim), dtype=np.float32)
    d, g = ix.search(z, 5)                         # zero query: distance exactly 1 to everything, lowest ids first
    assert np.all(d == 1.0) and g.tolist() == [[0, 1, 2, 3, 4]] * 2
    bad_q = rng.standard_normal((2, dim), dtype=np.float32)
    bad_q[0, 3] = np.nan
    bad_q[1, 9] = -np.inf
    d, g = ix.search(bad_q, 5)                     # a non-finite query is the zero query
    assert np.all(d == 1.0) and g.tolist() == [[0, 1, 2, 3, 4]] * 2
    zr = clip_lib.Index(clip, dim, "i8")           # zero and non-finite rows: distance exactly 1 to any query
    zr.add(rows[:600])
    d, g = zr.search(rng.standard_normal((4, dim), dtype=np.float32), 1024)
    for r in (500, 501, 502, 503):
        assert np.all((g == r).sum(1) == 1) and np.all(d[g == r] == 1.0)
    assert np.all(g[:, 600:] == -1) and np.all(d[:, 600:] == np.inf)
    zr.close()
    small = clip_lib.Index(clip, dim, "i8")
    small.add(rows[:3])
    d, g = small.search(rows[:2], 10)
    assert np.all(g[:, 3:] == -1) and np.all(d[:, 3:] == np.inf) and sorted(g[0, :3].tolist()) == [0, 1, 2]
    empty = clip_lib.Index(clip, dim, "i8")
    d, g = empty.search(rows[:2], 3)
    assert np.all(g == -1) and np.all(d == np.inf)
    for x in (ix, small, empty):
        x.close()


def test_device_forms_match_host_forms(clip, clip_lib):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    rng = np.random.default_rng(9)
    dim, n, nq, k = 512, 20000, 37, 50
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    host = clip_lib.Index(clip, dim, "i8")
    host.add(rows)
    hd, hi = host.search(q, k)
    dev = clip_lib.Index(clip, dim, "i8")
    tr, tq = torch.from_numpy(rows).cuda(), torch.from_numpy(q).cuda()
    td = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dev.add_device(tr.data_ptr(), 7001)
    dev.add_device(tr[7001:].data_ptr(), n - 7001)
    dev.search_device(tq.data_ptr(), nq, k, td.data_ptr(), ti.data_ptr())
    clip.synchronize()
    assert len(dev) == n
    assert np.array_equal(td.cpu().numpy().view(np.uint32), hd.view(np.uint32)) and np.array_equal(ti.cpu().numpy(), hi)
    host.close()
    dev.close()


def test_bit_identity_across_splits_and_save_load(clip, clip_lib, tmp_path):
    rng = np.random.default_rng(21)
    dim, n, nq, k = 768, 50000, 300, 100
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    a = clip_lib.Index(clip, dim, "i8")
    a.add(rows)
    d1, i1 = a.search(q, k)
    d2, i2 = a.search(q, k)
    assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32)) and np.array_equal(i1, i2)
    parts = [a.search(q[s], k) for s in (slice(0, 17), slice(17, 200), slice(200, 300))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]).view(np.uint32), d1.view(np.uint32))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), i1)
    b = clip_lib.Index(clip, dim, "i8")
    cuts = [0, 1, 1023, 1030, 4097, 31000, n]      # crosses the 1024-row first allocation and the doublings after it
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b.add(rows[lo:hi])
        b.search(q[:3], 7)                         # interleaved searches do not disturb later results
    d3, i3 = b.search(q, k)
    assert np.array_equal(d3.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i3, i1)
    p1, p2 = str(tmp_path / "a.index"), str(tmp_path / "b.index")
    a.save(p1)
    assert os.path.getsize(p1) == 28 + n * dim
    assert struct.unpack("<IIIQ", open(p1, "rb").read(28)[8:]) == (1, dim, I8, n)
    c = clip_lib.Index.load(clip, p1)
    assert len(c) == n and c.dim == dim
    d4, i4 = c.search(q, k)
    assert np.array_equal(d4.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i4, i1)
    c.add(rows[:5])                                # a loaded index grows like any other
    assert len(c) == n + 5
    d5, i5 = c.search(rows[:1], 1)
    assert i5[0, 0] == 0
    c.save(p2)
    assert open(p2, "rb").read()[28 + n * dim:] == open(p1, "rb").read()[28:28 + 5 * dim]
    c.close()
    c = clip_lib.Index.load(clip, p1)
    c.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    b.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    for x in (a, b, c):
        x.close()


def test_malformed_i8_files(clip, clip_lib, tmp_path, capfd):
    L = clip_lib.lib()
    rng = np.random.default_rng(3)
    dim = 32
    ix = clip_lib.Index(clip, dim, "i8")
    ix.add(rng.standard_normal((10, dim), dtype=np.float32))
    good = str(tmp_path / "good.index")
    ix.save(good)
    raw = open(good, "rb").read()
    assert len(raw) == 28 + 10 * dim

    def bad(name, data, msg):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        assert not L.clip_amd_index_load(clip.ctx, p.encode())
        assert msg in capfd.readouterr().err

    hdr = lambda d=dim, dt=I8, n=10: b"CLIPIDX1" + struct.pack("<IIIQ", 1, d, dt, n)
    bad("trunc.index", raw[:-1], "its header says")
    bad("long.index", raw + b"\0", "its header says")
    bad("f16size.index", hdr() + raw[28:] * 2, "its header says")     # an f16 payload under an i8 header
    bad("rows.index", hdr(n=11) + raw[28:], "its header says")
    bad("dtype2.index", hdr(dt=2) + raw[28:], "dtype 2")
    ok = clip_lib.Index.load(clip, good)
    d0, i0 = ix.search(np.ones((1, dim), np.float32), 3)
    d1, i1 = ok.search(np.ones((1, dim), np.float32), 3)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i0, i1)
    with pytest.raises(ValueError):
        clip_lib.Index(clip, dim, "int8")
    ok.close()
    ix.close()


def _recall_at_10(clip, clip_lib, rows, q):
    got = {}
    for dt in ("f32", "i8"):
        ix = clip_lib.Index(clip, rows.shape[1], dt)
        ix.add(rows)
        got[dt] = ix.search(q, 10)[1]
        ix.close()
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / 10.0 for a, b in zip(got["f32"], got["i8"])]))


def test_recall_against_f32(clip, clip_lib):
    rng = np.random.default_rng(2024)
    n, dim, nq = 20000, 512, 200
    gauss = rng.standard_normal((n, dim), dtype=np.float32)
    r_gauss = _recall_at_10(clip, clip_lib, gauss, rng.standard_normal((nq, dim), dtype=np.float32))
    centres = rng.standard_normal((100, dim), dtype=np.float32)
    lab = rng.integers(0, 100, n)
    clustered = (centres[lab] + rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
    qc = (centres[rng.integers(0, 100, nq)] + rng.standard_normal((nq, dim), dtype=np.float32)).astype(np.float32)
    r_clust = _recall_at_10(clip, clip_lib, clustered, qc)
    print("recall@10 i8 vs f32: gaussian %.4f clustered %.4f" % (r_gauss, r_clust))
    assert r_gauss >= 0.95 and r_clust >= 0.95, (r_gauss, r_clust)


def test_one_million_rows(clip, clip_lib, tmp_path):
    torch = pytest.importorskip("torch")
    dim, n, nq, k = 512, 1 << 20, 64, 100
    ix = clip_lib.Index(clip, dim, "i8")
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
    check(dist[sub], ids[sub], ref_distances(rows, quantize(q[sub])), k, dim)
    ix.close()
    os.remove(str(tmp_path / "big.index"))
