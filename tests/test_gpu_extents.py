"""GPU tier of the extents of a labelling (k_extents.hip, clip_amd_index_extents).  The oracle is the numpy reference of
tests/extents_common.py over the library's own pair list: `Index.pairs(4.0)` lists every pair whose distance is not NaN with the bits the
contract names, and every output is a maximum or minimum over those values, so every comparison here is for equality of bits.
Sizes: 333 rows (three row tiles, the last one partial) at dim 512 and at dim 72 (rows that end in a chunk of fewer than 4 k-steps), each
with f16 / f32 / i8; labellings: components, random with -1, one group, all single, exact copies; then masks (remove + allow against a
fresh index), the tile skip (640 rows, counts from the hook), the device form, determinism, save / load, refusals, and the two commands
of image_search that print extents."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from extents_common import clustered, reference, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("f16", "f32", "i8")
N = 333
SHAPES = [(dtype, dim) for dim in (512, 72) for dtype in DTYPES]


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
    """per (dtype, dim): the index of N clustered rows, its whole pair list, and the labels of components at a radius with both kinds of
    group; built once, shared by the tests, never changed"""
    built = {}

    def get(dtype, dim):
        if (dtype, dim) not in built:
            rng = np.random.default_rng(dim + len(dtype))
            ix = clip_lib.Index(clip, dim, dtype)
            ix.add(clustered(rng, N, dim))
            pairs = ix.pairs(4.0)
            assert len(pairs[0]) == N * (N - 1) // 2
            radius = float(np.quantile(pairs[2], 0.02))
            comp = ix.components(radius)[0]
            sizes = np.bincount(comp, minlength=N)
            assert (sizes >= 2).sum() >= 3 and (sizes == 1).sum() >= 3          # multi-row groups and singletons
            built[(dtype, dim)] = (ix, pairs, comp)
        return built[(dtype, dim)]
    yield get
    for ix, _, _ in built.values():
        ix.close()


def check(ix, labels, pairs, allow=None, eligible=None):
    got = ix.extents(labels, allow=allow)
    want = reference(len(ix), labels, *pairs, eligible=eligible)
    assert same_bits(got, want[:5]), [int((np.asarray(g) != np.asarray(w)).sum()) for g, w in zip(got, want)]
    return got, want[5]


@pytest.mark.parametrize("dtype,dim", SHAPES)
def test_labellings_equal_the_reference_over_pairs(cases, dtype, dim):
    ix, pairs, comp = cases(dtype, dim)
    rng = np.random.default_rng(7)
    got, groups = check(ix, comp, pairs)                                       # components: chains and singletons
    assert groups == len(np.unique(comp))
    single = np.bincount(comp, minlength=N)[comp] == 1
    assert np.all(got[3][single] == 0) and np.all(got[4][single] == -1) and np.all(got[0][single] == np.flatnonzero(single))
    assert np.all(got[2] >= got[1]) and np.all(got[3] <= got[2]) and np.all(got[3] >= got[1])       # radius <= reach <= diameter
    labels = rng.integers(0, N, N).astype(np.int64)                             # random labels in [0, size), some -1
    labels[rng.random(N) < 0.15] = -1
    labels[:40] = rng.integers(0, 6, 40)                                        # a few larger groups too
    got, _ = check(ix, labels, pairs)
    assert np.all(got[0][labels < 0] == -1) and np.all(np.isposinf(got[3][labels < 0])) and np.all(got[4][labels < 0] == -1)
    got, groups = check(ix, np.full(N, N - 1, dtype=np.int64), pairs)          # one group of all rows
    assert groups == 1 and len(np.unique(got[0])) == 1 and got[2][0] == pairs[2].max()
    got, groups = check(ix, rng.permutation(N).astype(np.int64), pairs)        # all singletons, none labelled by itself necessarily
    assert groups == N and np.array_equal(got[0], np.arange(N)) and not got[1].any() and not got[2].any() and np.all(got[4] == -1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_copies_resolve_ties_to_the_lowest_id(clip, clip_lib, dtype):
    rng = np.random.default_rng(11)
    dim, copies = 72, 7
    heads = rng.standard_normal((N // copies + 1, dim)).astype(np.float32)
    of = rng.permutation(np.repeat(np.arange(len(heads)), copies)[:N])          # row -> the vector it copies, shuffled over the rows
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(heads[of])
    pairs = ix.pairs(4.0)
    labels = np.array([np.flatnonzero(of == of[x])[-1] for x in range(N)], dtype=np.int64)       # labelled by the group's HIGHEST id
    (centre, radius, diameter, reach, far), groups = check(ix, labels, pairs)
    lowest = np.array([np.flatnonzero(of == of[x])[0] for x in range(N)])
    size = np.bincount(of)[of]
    assert groups == len(np.unique(of)) and np.array_equal(centre, lowest)      # every reach of a group is one value: the lowest id wins
    second = np.array([np.flatnonzero(of == of[x])[min(1, size[x] - 1)] for x in range(N)])
    assert np.array_equal(far[size > 1], np.where(lowest == np.arange(N), second, lowest)[size > 1])  # all equally far: the lowest other id
    assert np.all(radius == diameter) and np.all(np.abs(reach) < 1e-3)
    ix.close()


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
    labels = rng.integers(0, 12, N).astype(np.int64) * 25                       # labels that may be removed rows or rows of another group
    labels[rng.random(N) < 0.1] = -1
    labels[np.flatnonzero(~allow)[:5]] = N + 1000                               # a row that is not allowed may carry anything
    got = ix.extents(labels, allow=allow)
    fresh = clip_lib.Index(clip, dim, dtype)
    fresh.add(rows[keep])
    new_id = np.full(N, -1, dtype=np.int64)
    new_id[keep] = np.arange(len(keep))
    _, inverse = np.unique(labels[keep], return_inverse=True)                   # labels mapped in order; -1 stays the smallest
    mapped = inverse.astype(np.int64) - (1 if (labels[keep] < 0).any() else 0)
    want = fresh.extents(mapped)
    assert same_bits([got[1][keep], got[2][keep], got[3][keep]], want[1:4])
    for mine, fresh_ids in ((got[0][keep], want[0]), (got[4][keep], want[4])):      # ids mapped in order
        assert np.array_equal(np.where(mine >= 0, new_id[mine], -1), fresh_ids)
    out = np.flatnonzero(~eligible)
    assert np.all(got[0][out] == -1) and np.all(got[4][out] == -1) and all(np.all(np.isposinf(a[out])) for a in got[1:4])
    pairs = fresh.pairs(4.0)
    assert same_bits(want, reference(len(keep), mapped, *pairs)[:5])
    ix.close()
    fresh.close()


@pytest.mark.parametrize("dtype", ("f16", "i8"))
def test_tile_skip_computes_fewer_tiles_and_the_same_bits(clip, clip_lib, dtype):
    n, dim = 640, 72                                                            # five tiles of 128 rows: fifteen tile pairs
    rng = np.random.default_rng(9)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(clustered(rng, n, dim))
    pairs = ix.pairs(4.0)
    assert ix.extents_route(0) == 0                                             # no call yet
    sorted_labels = np.arange(n, dtype=np.int64) // 64
    shuffled = rng.permutation(sorted_labels)
    for labels, expect in ((sorted_labels, lambda c: c == 5), (shuffled, lambda c: 5 < c <= 15)):
        ix.extents_route(0)
        skipping = ix.extents(labels)
        computed = ix.extents_route(1)
        assert expect(computed), computed
        every = ix.extents(labels)
        assert ix.extents_route(0) == 15
        assert same_bits(skipping, every) and same_bits(every, reference(n, labels, *pairs)[:5])
    with pytest.raises(ValueError):
        ix.extents_route(2)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form_determinism_and_save_load(clip, clip_lib, cases, tmp_path, dtype):
    import torch
    ix, pairs, comp = cases(dtype, 72)
    rng = np.random.default_rng(13)
    labels = np.where(rng.random(N) < 0.1, -1, comp)
    allow = rng.random(N) < 0.8
    first = ix.extents(labels, allow=allow)
    assert same_bits(first, ix.extents(labels, allow=allow))                    # run to run
    p = str(tmp_path / "rows.index")
    ix.save(p)
    loaded = clip_lib.Index.load(clip, p)
    assert same_bits(first, loaded.extents(labels, allow=allow))                # across save / load
    loaded.close()
    tl = torch.from_numpy(labels).cuda()
    tw = torch.from_numpy(clip_lib.allow_words(allow, N).view(np.int64).copy()).cuda()
    ids = [torch.full((N,), -7, dtype=torch.int64, device="cuda") for _ in range(2)]
    flt = [torch.full((N,), -7, dtype=torch.float32, device="cuda") for _ in range(3)]
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.extents_device(tl.data_ptr(), ids[0].data_ptr(), flt[0].data_ptr(), flt[1].data_ptr(), flt[2].data_ptr(), ids[1].data_ptr(),
                      count.data_ptr(), d_allow=tw.data_ptr())
    clip.synchronize()
    got = (ids[0].cpu().numpy(), flt[0].cpu().numpy(), flt[1].cpu().numpy(), flt[2].cpu().numpy(), ids[1].cpu().numpy())
    assert same_bits(got, first)
    assert int(count.item()) == reference(N, labels, *pairs, eligible=allow)[5] == len(np.unique(labels[allow & (labels >= 0)]))
    ids[0].fill_(-7)
    torch.cuda.synchronize()
    ix.extents_device(tl.data_ptr(), ids[0].data_ptr())                         # centre only, every row eligible
    clip.synchronize()
    assert np.array_equal(ids[0].cpu().numpy(), ix.extents(labels)[0]) and float(flt[0][0]) == float(first[1][0])


def test_refused_calls_leave_poisoned_outputs_untouched(clip, clip_lib, cases, capfd):
    ix, pairs, comp = cases("f16", 72)
    L = clip_lib.lib()
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    ids = [np.full(N, -7, dtype=np.int64) for _ in range(2)]
    flt = [np.full(N, -7, dtype=np.float32) for _ in range(3)]
    out = (ids[0].ctypes.data_as(i64p), flt[0].ctypes.data_as(f32p), flt[1].ctypes.data_as(f32p), flt[2].ctypes.data_as(f32p),
           ids[1].ctypes.data_as(i64p))
    labels = comp.copy()
    labels[200] = N                                                             # a member's label >= size
    capfd.readouterr()
    assert L.clip_amd_index_extents(ix.handle, labels.ctypes.data_as(i64p), None, *out) == -1
    assert "label %d of row 200" % N in capfd.readouterr().err
    assert L.clip_amd_index_extents(ix.handle, None, None, *out) == -1
    assert L.clip_amd_index_extents(ix.handle, comp.ctypes.data_as(i64p), None, None, *out[1:]) == -1
    assert L.clip_amd_index_extents(None, comp.ctypes.data_as(i64p), None, *out) == -1
    assert L.clip_amd_index_extents_device(ix.handle, None, None, 1, None, None, None, None, None) is False
    assert L.clip_amd_index_extents_device(ix.handle, 1, None, None, None, None, None, None, None) is False
    assert all(np.all(a == -7) for a in ids + flt)
    with pytest.raises(ValueError):
        ix.extents(labels)
    allow = np.ones(N, dtype=bool)
    allow[200] = False                                                          # the same label on a row that is not eligible is fine
    words = clip_lib.allow_words(allow, N)
    groups = L.clip_amd_index_extents(ix.handle, labels.ctypes.data_as(i64p), words.ctypes.data_as(C.POINTER(C.c_uint64)), *out)
    want = reference(N, labels, *pairs, eligible=allow)
    assert groups == want[5] and same_bits((ids[0], flt[0], flt[1], flt[2], ids[1]), want[:5])
    assert L.clip_amd_index_extents(ix.handle, comp.ctypes.data_as(i64p), None, out[0], None, None, None, None) == len(np.unique(comp))
    empty = clip_lib.Index(clip, 72, "f16")
    ids[0][:] = -7
    assert L.clip_amd_index_extents(empty.handle, comp.ctypes.data_as(i64p), None, *out) == 0 and np.all(ids[0] == -7)
    assert all(a.size == 0 for a in empty.extents([]))
    empty.close()


# ---- image_search groups --extents / dedup --extents ----

def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


@pytest.fixture(scope="module")
def db(tmp_path_factory, fixture_cache):
    """the seventeen-image tree of tests/test_gpu_image_search_groups.py: ten images, five byte-identical copies, two noisy copies"""
    from PIL import Image
    from oracle import fixtures
    base = tmp_path_factory.mktemp("extents")
    imgs = base / "pictures"
    rng = np.random.default_rng(12)
    originals, arrays = [], []
    for i in range(10):
        os.makedirs(imgs / "orig", exist_ok=True)
        arr = rng.integers(0, 256, size=(int(rng.integers(24, 64)), int(rng.integers(24, 64)), 3), dtype=np.uint8)
        p = imgs / "orig" / ("img%d.png" % i)
        Image.fromarray(arr).save(p, format="PNG")
        originals.append(p)
        arrays.append(arr)
    for src, dst in ((0, "copies/a/x0.png"), (0, "copies/b/y0.png"), (3, "copies/a/x3.png"), (7, "z/z7.png"), (7, "z/zz7.png")):
        os.makedirs((imgs / dst).parent, exist_ok=True)
        shutil.copy(originals[src], imgs / dst)
    for src, dst in ((2, "zz_noisy/n2.png"), (7, "zz_noisy/n7.png")):
        os.makedirs((imgs / dst).parent, exist_ok=True)
        noisy = np.clip(arrays[src].astype(np.int16) + rng.integers(-8, 9, size=arrays[src].shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(imgs / dst, format="PNG")
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    out = base / "db"
    r = run("build", "-m", model, "-v", "0", "--dtype", "f32", "--db", out, imgs)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    paths = (out / "images.paths").read_text().split("\n")[1:-1]
    assert len(paths) == 17
    return dict(db=out, base=base, paths=paths, model=model)


def extent_lines(found, paths):
    lines = []
    for g, (c, radius, diameter, members) in enumerate(found):
        lines += ([""] if g else []) + ["  %f %f %s" % (radius, diameter, paths[c])] + ["  %f %s" % (d, paths[i]) for i, d in members]
    return lines


def test_image_search_prints_extents_and_prunes_to_the_centres(db, clip_lib):
    from clip_cpp_amd import image_search
    paths = db["paths"]
    n = len(paths)
    clip = clip_lib.Clip(db["model"], verbosity=0)
    index = clip_lib.Index.load(clip, str(db["db"] / "images.index"))
    lo, hi, d = index.linkage()
    tree_labels = clip_lib.cut_linkage(n, lo, hi, d, n_groups=5)
    tree_found = image_search.extent_groups(tree_labels, *index.extents(tree_labels)[:4], 1, largest_first=True)
    plain, kept, cut = image_search.tree_groups(n, lo, hi, d, 5, min_size=1)
    radius = "%.9g" % image_search.tree_groups(n, lo, hi, d, 12)[1]             # dedup at the longest link kept: the groups of `groups -n 12`
    comp, nearest, _ = index.components(float(radius))
    comp_found = image_search.extent_groups(comp, *index.extents(comp)[:4], 2)
    comp_plain = image_search.component_groups(comp, nearest)
    index.close()
    clip.close()
    assert len(comp_found) == len(comp_plain) >= 2 and any(len(m) >= 2 for _, _, _, m in comp_found)

    r = run("groups", "--db", db["db"], "-n", 5, "--min", 1, "--extents")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    closing = ("main: 5 groups, 5 of them with at least 1 images, %d images in those; longest link kept %f, cut at %f" % (n, kept, cut))
    assert lines[lines.index("groups:") + 1:-1] == extent_lines(tree_found, paths)
    assert lines[-1] == closing + "; largest diameter %f" % max(g[2] for g in tree_found)
    assert [sorted([c] + [i for i, _ in m]) for c, _, _, m in tree_found] == [sorted(i for i, _ in g) for g in plain]     # the same groups
    r = run("groups", "--db", db["db"], "-n", 5, "--min", 1)                    # without the flag: what it always printed
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    want = []
    for g, members in enumerate(plain):
        want += ([""] if g else []) + ["  %f %s" % (dist, paths[i]) for i, dist in members]
    assert lines[lines.index("groups:") + 1:-1] == want and lines[-1] == closing

    r = run("dedup", "--db", db["db"], "-d", radius, "--extents")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[lines.index("duplicate groups:") + 1:-1] == extent_lines(comp_found, paths)
    members = sum(1 + len(m) for _, _, _, m in comp_found)
    assert lines[-1] == "main: %d groups, %d images, largest diameter %f" % (len(comp_found), members, max(g[2] for g in comp_found))
    r = run("dedup", "--db", db["db"], "-d", radius)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    want = []
    for g, group in enumerate(comp_plain):
        want += ([""] if g else []) + ["  %f %s" % (dist, paths[i]) for i, dist in group]
    assert lines[lines.index("duplicate groups:") + 1:-1] == want and lines[-1] == "main: %d groups, %d images" % (len(comp_plain), members)

    pruned = db["base"] / "pruned"
    shutil.copytree(db["db"], pruned)
    r = run("dedup", "--prune", "--extents", "-v", 0, "--db", pruned, "-d", radius)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    gone = {i for _, _, _, m in comp_found for i, _ in m}
    assert r.stdout.splitlines()[-1] == "main: %d removed, %d kept, largest diameter %f" % (len(gone), n - len(gone), max(g[2] for g in comp_found))
    left = (pruned / "images.paths").read_text().split("\n")[1:-1]
    assert left == [p for i, p in enumerate(paths) if i not in gone] and all(paths[c] in left for c, _, _, _ in comp_found)

    gridded = db["base"] / "gridded"
    shutil.copytree(db["db"], gridded)
    (gridded / "images.regions").write_text("grid 2\n")
    for argv in (("groups", "--db", gridded, "-n", 5, "--extents"), ("dedup", "--db", gridded, "--extents")):
        r = run(*argv)
        assert r.returncode == 1 and "`%s` does not support such a database yet" % argv[0] in r.stderr
