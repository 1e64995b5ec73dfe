"""End to end: `python -m clip_cpp_amd.image_search eval` over the small database of tests/test_gpu_image_search_file.py (its fixtures are
reused).  The expected figures come from Index.search over the same database: a pair's rank is the position of its image in the complete
ranking of its caption, encoded in the batch `eval` encodes it in; recall@K, median rank and MRR are then formed here in float64."""
import shutil

import numpy as np
import pytest

from test_gpu_image_search_file import cli, db, library  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CAPTIONS = ["a red apple", "noise", "a photo of a cat", "colourful static", "an apple on a table", "a dog", "pixels"]


def test_eval_figures_and_worst_pairs(cli, db, capfd, tmp_path):
    paths, index, clip = db["paths"], db["index"], db["clip"]
    targets = [7, 0, 3, 7, 10, 3, 5]                           # paths occur twice
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("".join("%s\t%s\n" % (c, paths[t]) for c, t in zip(CAPTIONS, targets)))
    vecs = clip.encode_texts([clip.tokenize(c) for c in CAPTIONS], normalize=True)
    for prefix in (None, paths[0][:paths[0].rindex("/")]):
        allow = None if prefix is None else np.array([p.startswith(prefix) for p in paths])
        D0, I0 = index.search(vecs, len(paths))
        D, I = index.search(vecs, len(paths), allow=allow)
        d = np.array([D0[i, list(I0[i]).index(t)] for i, t in enumerate(targets)])
        rank = np.array([np.count_nonzero((I[i] >= 0) & ((D[i] < d[i]) | ((D[i] == d[i]) & (I[i] < t)))) for i, t in enumerate(targets)]) + 1.0
        rc, out, err = cli(capfd, "eval", "--db", db["dir"], "-n", 3, *([] if prefix is None else ["--in", prefix]), pairs)
        assert rc == 0, out[-3000:] + err[-3000:]
        lines = out.split("\n")
        at = lines.index("retrieval:")
        assert lines[at + 1] == "  recall@1 %f recall@5 %f recall@10 %f" % tuple(float(np.mean(rank <= k)) for k in (1, 5, 10))
        assert lines[at + 2] == "  median rank %.1f mean reciprocal rank %f" % (float(np.median(rank)), float(np.mean(1.0 / rank)))
        worst = sorted(range(len(targets)), key=lambda i: (-rank[i], i))[:3]
        assert lines[at + 3] == "worst placed:"
        assert lines[at + 4:at + 7] == ["  %d %f %s %s" % (rank[i], d[i], paths[targets[i]], CAPTIONS[i]) for i in worst]
        assert lines[at + 7] == "main: %d pairs ranked among %d images" % (len(targets), len(paths) if allow is None else int(allow.sum()))


def test_eval_refusals(cli, db, capfd, tmp_path):
    from clip_cpp_amd import image_search
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("a red apple\t%s\na dog\tnot/indexed.png\n" % db["paths"][0])
    rc, out, err = cli(capfd, "eval", "--db", db["dir"], pairs)
    assert rc == 1 and "line 2" in out + err and "not/indexed.png" in out + err
    gridded = tmp_path / "gridded"
    shutil.copytree(db["dir"], gridded)
    (gridded / image_search.REGIONS_FILE).write_text("")      # what a --grid build leaves: the refusal looks no further
    pairs.write_text("a red apple\t%s\n" % db["paths"][0])
    rc, out, err = cli(capfd, "eval", "--db", gridded, pairs)
    assert rc == 1 and "--grid" in out + err and "eval" in out + err
