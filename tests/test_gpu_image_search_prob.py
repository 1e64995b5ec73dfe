"""End to end: `image_search label --prob` and `search --prob` over the small database of tests/test_gpu_image_search_file.py (its fixtures
are reused) print the probabilities of Index.softmax_index / Index.softmax over the same database, in the order the commands print
without --prob; and Clip.zero_shot_top ranks more labels than zero_shot_label_images accepts."""
import numpy as np
import pytest

from test_gpu_image_search_file import cli, db, library  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAMES = ["a red apple", "noise", "a photo of a cat", "colourful static", "a dog"]


def test_prob_lines_and_zero_shot_top(cli, db, clip_lib, capfd):
    paths, index, clip = db["paths"], db["index"], db["clip"]
    # label --prob: per image "  distance probability label", the labels in the order of the run without --prob
    labels = clip_lib.Index(clip, index.dim, "f32")
    labels.add(clip.encode_texts([clip.tokenize(t) for t in NAMES], normalize=True))
    dist, ids, probs, _ = labels.softmax_index(index, 3, scale=50.0)
    rc, out, err = cli(capfd, "label", "--db", db["dir"], "-v", 0, "-n", 3, "--prob", "--scale", 50, *NAMES)
    assert rc == 0, out[-3000:] + err[-3000:]
    want = [["  %f %f %s" % (d, p, NAMES[j]) for d, p, j in zip(dist[i], probs[i], ids[i])] for i in range(len(paths))]
    got = [block.split("\n")[1:] for block in out[:out.index("main:")].strip("\n").split("\n\n")]
    assert got == want
    rc, plain, err = cli(capfd, "label", "--db", db["dir"], "-v", 0, "-n", 3, *NAMES)
    assert rc == 0 and [ln.split(" ", 4)[4] for b in got for ln in b] == [ln.split(" ", 3)[3] for ln in plain.split("\n") if ln.startswith("  ")]
    labels.close()
    # search --prob: "  distance probability path" and the query's log Z, with --in; refused with -d
    prefix = paths[0][:paths[0].rindex("/")]
    allow = np.array([p.startswith(prefix) for p in paths])
    vec = np.asarray(clip.encode_text(clip.tokenize(NAMES[0]), normalize=True), dtype=np.float32)
    dist, ids, probs, log_z = index.softmax(vec[None, :], 4, allow=allow)
    rc, out, err = cli(capfd, "search", "--db", db["dir"], "-v", 0, "-n", 4, "--in", prefix, "--prob", NAMES[0])
    assert rc == 0, out[-3000:] + err[-3000:]
    hits = [(d, p, i) for d, p, i in zip(dist[0], probs[0], ids[0]) if i >= 0]
    assert out.split("\n")[:len(hits) + 1] == ["  %f %f %s" % (d, p, paths[i]) for d, p, i in hits] + ["main: log Z %f at scale 100" % log_z[0]]
    rc, plain, err = cli(capfd, "search", "--db", db["dir"], "-v", 0, "-n", 4, "--in", prefix, NAMES[0])
    assert [ln.split(" ", 3)[3] for ln in plain.split("\n") if ln.startswith("  ")] == [paths[i] for _, _, i in hits]
    assert cli(capfd, "search", "--db", db["dir"], "--prob", "-d", 0.5, NAMES[0])[0] == 1
    # zero_shot_top with more labels than zero_shot_label_images takes: per image the ids of search over the label index
    many = ["label %d" % i for i in range(8200)]
    images = [np.random.default_rng(i).integers(0, 256, size=(32, 40, 3), dtype=np.uint8) for i in range(3)]
    probs, top, log_z = clip.zero_shot_top(images, many, top=5)
    labels = clip_lib.Index(clip, index.dim, "f32")
    for b in range(0, len(many), 1024):
        labels.add(clip.encode_texts([clip.tokenize(t) for t in many[b:b + 1024]], normalize=True))
    assert np.array_equal(top, labels.search(clip.encode_images_u8(images), 5)[1]) and top.shape == (3, 5)
    assert np.all(probs > 0) and np.all(np.diff(probs, axis=1) <= 0) and np.all(np.isfinite(log_z))
    labels.close()
