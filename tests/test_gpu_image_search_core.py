"""End to end: `python -m clip_cpp_amd.image_search groups --core K` / `levels --core K` over a small synthetic database: two bursts of
near-identical rows joined by a thin chain of stray rows, and one row far from everything.  The single-linkage tree cannot tell the bursts
apart (`groups -n 2` splits off the far row and leaves everything else chained into one group); the mutual-reachability tree can
(`groups --core 5 -n 2` files each burst on its own and leaves the middle of the chain and the far row unfiled).  Both facts are first
established in numpy, then asked of the command line.  `levels --core K` prints level_rows over Index.linkage_core; the refusal when no
distance gives N groups; without --core both commands print what they print from Index.linkage."""
import os
import subprocess
import sys

import numpy as np
import pytest

from linkage_core_common import core_distances, core_kruskal, kruskal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, BURST, CHAIN, K = 32, 15, 5, 5


def run(*args):
    return subprocess.run([sys.executable, "-m", "clip_cpp_amd.image_search"] + [str(a) for a in args], capture_output=True, text=True,
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)


def bridged_rows():
    """(rows f32 [36, DIM], kind [36]): kind 0 / 1 the two bursts (unit vectors a and b at a right angle, noise 0.01 per coordinate: two
    rows of a burst are at about 0.003), 2 the chain (five rows in steps of pi / 12 along the arc from a to b: one step is 0.034, two
    steps 0.134, three steps 0.293), 3 the far row (at a right angle to both: about 1 from everything); ids shuffled.
    With K = 5 the core distance of a burst row is about 0.003; of the chain's first and last row 0.034 (a burst is one step away); of
    its second and fourth 0.134 (two neighbours at one step, the burst at two); of the middle row 0.293 (four chain rows, then a burst at
    three steps).  So between 0.134 and 0.293 the cut is: either burst with its two chain rows, the middle row and the far row alone;
    both links of the middle row weigh its core distance, so from there on everything but the far row is one group."""
    rng = np.random.default_rng(7)
    a, b, c = np.eye(DIM)[0], np.eye(DIM)[1], np.eye(DIM)[2]
    rows = [a + 0.01 * rng.standard_normal(DIM) for _ in range(BURST)] + [b + 0.01 * rng.standard_normal(DIM) for _ in range(BURST)]
    rows += [np.cos(t * np.pi / 12) * a + np.sin(t * np.pi / 12) * b for t in range(1, CHAIN + 1)] + [c]
    kind = np.array([0] * BURST + [1] * BURST + [2] * CHAIN + [3])
    order = rng.permutation(len(rows))
    return np.asarray(rows, dtype=np.float32)[order], kind[order]


@pytest.fixture(scope="module")
def db(tmp_path_factory, fixture_cache, clip_lib):
    from oracle import fixtures
    rows, kind = bridged_rows()
    out = tmp_path_factory.mktemp("core") / "db"
    os.makedirs(out)
    model = fixtures.cached_model(fixture_cache, "tiny", "f32")
    clip = clip_lib.Clip(model, verbosity=0)
    index = clip_lib.Index(clip, DIM, "f32")
    index.add(rows)
    index.save(str(out / "images.index"))
    trees = dict(plain=index.linkage(), core=index.linkage_core(K), inside=index.linkage_core(K, allow=kind != 3))
    index.close()
    clip.close()
    paths = ["%s/img%02d.png" % (("left", "right", "chain", "far")[g], i) for i, g in enumerate(kind)]
    (out / "images.paths").write_text("".join(p + "\n" for p in [model] + paths))
    return dict(db=out, rows=rows, kind=kind, paths=paths, trees=trees)


def printed_groups(stdout, heading="groups:"):
    lines = stdout.splitlines()
    k = lines.index(heading) + 1
    assert lines[-1].startswith("main: ")
    groups = [[]]
    for line in lines[k:-1]:
        if line == "":
            groups.append([])
        else:
            dist, path = line.strip().split(" ", 1)
            groups[-1].append((dist, path))
    return [g for g in groups if g], lines[-1]


def test_the_numpy_oracle_separates_the_bursts_only_with_core_distances(clip_lib):
    rows, kind = bridged_rows()
    n = len(rows)
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    i, j = np.triu_indices(n, 1)
    d = (1.0 - np.einsum("ij,ij->i", unit[i], unit[j])).astype(np.float32)
    lo, hi, dd = kruskal(n, i, j, d)
    labels = clip_lib.cut_linkage(n, lo, hi, dd, n_groups=2)
    far = int(np.flatnonzero(kind == 3)[0])
    assert labels[far] == far and len(np.unique(labels[kind != 3])) == 1           # the far row alone, the bursts chained into one group
    core = core_distances(n, i, j, d, K)
    lo, hi, w = core_kruskal(n, i, j, d, core)
    labels, radius = clip_lib.cut_linkage_sized(n, lo, hi, w, 2)
    left, right = np.unique(labels[kind == 0]), np.unique(labels[kind == 1])
    assert len(left) == 1 and len(right) == 1 and left[0] != right[0]              # each burst whole, the two apart
    sizes = np.bincount(labels, minlength=n)
    assert sorted(sizes[sizes >= 2].tolist()) == [BURST + 2, BURST + 2] and 0.12 < radius < 0.15       # (two chain rows on either side)
    assert labels[far] == far and int((sizes == 1).sum()) == 2


def test_groups_core_separates_what_groups_chains_together(db, clip_lib):
    from clip_cpp_amd.image_search import sized_groups, tree_groups
    paths, kind = db["paths"], db["kind"]
    n = len(paths)
    r = run("groups", "--db", db["db"], "-n", 2, "--min", 1)                       # the single-linkage tree
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    groups, closing = printed_groups(r.stdout)
    expect, kept, cut = tree_groups(n, *db["trees"]["plain"], 2, min_size=1)        # without --core: what it printed before
    assert groups == [[("%f" % dist, paths[i]) for i, dist in g] for g in expect]
    assert closing == "main: 2 groups, 2 of them with at least 1 images, %d images in those; longest link kept %f, cut at %f" % (n, kept, cut)
    assert [len(g) for g in groups] == [n - 1, 1] and groups[1][0][1].startswith("far/")
    both = {p.split("/")[0] for _, p in groups[0]}
    assert {"left", "right", "chain"} == both                                      # not separated

    r = run("groups", "--db", db["db"], "-n", 2, "--core", K)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    groups, closing = printed_groups(r.stdout)
    expect, radius, unfiled = sized_groups(n, *db["trees"]["core"][:3], 2)
    assert groups == [[("%f" % dist, paths[i]) for i, dist in g] for g in expect]
    assert closing == "main: 2 groups of at least 2 images, %d images in those; cut at radius %f, 2 images left unfiled" % (n - 2, radius)
    assert unfiled == 2 and len(groups) == 2
    sides = [{p.split("/")[0] for _, p in g} - {"chain"} for g in groups]
    assert sorted(map(sorted, sides)) == [["left"], ["right"]]                     # separated
    for g in groups:
        assert sum(p.startswith(("left/", "right/")) for _, p in g) == BURST

    r = run("groups", "--db", db["db"], "-n", 2, "--core", K, "--extents", "-v", 0)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert "groups:" not in lines and lines[-1].startswith(closing + "; largest diameter ")
    members = [line.split()[-1] for line in lines[:-1] if line]
    assert sorted(members) == sorted(p for g in groups for _, p in g)              # the same groups, measured

    r = run("groups", "--db", db["db"], "-n", 2, "--core", K, "--in", "left", "--in", "right", "--in", "chain")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    inside, closing = printed_groups(r.stdout)
    expect, radius, unfiled = sized_groups(n, *db["trees"]["inside"][:3], 2, eligible=kind != 3)
    assert inside == [[("%f" % dist, paths[i]) for i, dist in g] for g in expect] and unfiled == 1
    assert closing.endswith("cut at radius %f, 1 images left unfiled" % radius)


def test_groups_core_says_when_no_distance_gives_n_groups(db):
    r = run("groups", "--db", db["db"], "-n", 30, "--core", K)                     # 36 images cannot make 30 groups of two
    assert r.returncode == 1 and "groups:" not in r.stdout
    last = r.stdout.splitlines()[-1]
    assert last.startswith("main: -n 30: no distance of the tree gives 30 groups of at least 2 rows; the counts that occur: 1")
    assert " 30" not in last.split("occur:")[1]


def test_levels_core_prints_the_table_of_the_mutual_reachability_tree(db):
    from clip_cpp_amd.image_search import level_rows
    n = len(db["paths"])
    for flags, tree in (((), "plain"), (("--core", K), "core"), (("--core", 0), "plain")):
        table = level_rows(n, *db["trees"][tree][:3], 8)
        r = run("levels", "--db", db["db"], "-n", 8, *flags)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = r.stdout.splitlines()
        k = lines.index("levels:")
        assert lines[k + 1] == "distance groups images largest" and lines[-1] == "main: %d images, %d levels" % (n, len(table))
        assert [line.split() for line in lines[k + 2:-1]] == [["%f" % dist, str(g), str(i), str(m)] for dist, g, i, m in table]
        assert lines[-2].split()[1:] == ["1", str(n), str(n)]
    assert level_rows(n, *db["trees"]["core"][:3], 8) != level_rows(n, *db["trees"]["plain"], 8)
