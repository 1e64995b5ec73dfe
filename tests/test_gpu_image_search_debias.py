"""End to end: `python -m clip_cpp_amd.image_search debias`, `search --debias`, `eval --debias` and the stale-column rule of `update`, over
the small database of tests/test_gpu_image_search_file.py (its fixtures are reused).  Expected output comes from Index.hubness and
Index.search_biased over the same database."""
import shutil

import numpy as np
import pytest

from test_gpu_image_search_file import cli, db, library  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BANK = ["a red apple", "noise", "a photo of a cat", "colourful static", "an apple on a table", "a dog", "pixels"]


@pytest.mark.parametrize("mode", ["csls", "softmax"])
def test_debias_search_eval_and_stale_column(cli, db, library, clip_lib, capfd, tmp_path, mode):
    from clip_cpp_amd import image_search
    paths, index, clip = db["paths"], db["index"], db["clip"]
    d = tmp_path / "db"
    shutil.copytree(db["dir"], d)
    bank_file = tmp_path / "queries.txt"
    bank_file.write_text("\n".join(BANK) + "\n")
    # debias writes the column Index.hubness gives for the encoded lines
    rc, out, err = cli(capfd, "debias", "--db", d, "--mode", mode, "-k", 3, "--scale", 50, bank_file)
    assert rc == 0, out[-3000:] + err[-3000:]
    bank = clip_lib.Index(clip, index.dim, "f32")
    bank.add(clip.encode_texts([clip.tokenize(t) for t in BANK], normalize=True))
    want = index.hubness(bank, mode=mode, k=3, scale=50.0)
    bank.close()
    bias = image_search.read_bias(d, len(paths))
    assert bias.tobytes() == want.tobytes() and np.ptp(bias) > 0
    # search --debias prints search_biased's ranking: a text query under --in, and an indexed image
    prefix = paths[0][:paths[0].rindex("/")]
    allow = np.array([p.startswith(prefix) for p in paths])
    vec = np.asarray(clip.encode_text(clip.tokenize("a red apple"), normalize=True), dtype=np.float32)
    for args, (dist, scores, ids) in ((["--in", prefix, "a red apple"], index.search_biased(vec[None, :], 4, bias, allow=allow)),
                                      (["--like", paths[7]], index.search_ids_biased([7], 4, bias))):
        rc, out, err = cli(capfd, "search", "--db", d, "-n", 4, "--debias", *args)
        assert rc == 0, out[-3000:] + err[-3000:]
        lines = out.split("\n")
        at = lines.index("score distance path")
        want_lines = ["  %f %f %s" % (s, x, paths[i]) for s, x, i in zip(scores[0], dist[0], ids[0]) if i >= 0]
        assert len(want_lines) >= 3 and lines[at + 1:] == want_lines + [""]      # (fewer than -n under --in: the folder holds three)
    # eval --debias prints both recall lines
    targets = [7, 0, 3, 7, 10, 3, 5]
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("".join("%s\t%s\n" % (c, paths[t]) for c, t in zip(BANK, targets)))
    top = index.search_biased(clip.encode_texts([clip.tokenize(c) for c in BANK], normalize=True), 10, bias)[2]
    place = np.array([list(row).index(t) if t in row else 10 for row, t in zip(top, targets)])
    rc, out, err = cli(capfd, "eval", "--db", d, "--debias", pairs)
    assert rc == 0, out[-3000:] + err[-3000:]
    lines = out.split("\n")
    at = lines.index("retrieval:")
    assert lines[at + 1].startswith("  recall@1 ")
    assert lines[at + 2] == "  debiased recall@1 %f recall@5 %f recall@10 %f" % tuple(float(np.mean(place < k)) for k in (1, 5, 10))
    # update that adds an image deletes the column and says so; search --debias then refuses
    shutil.copy(library["base"] / "outside.jpg", library["imgs"] / "a" / "added.jpg")      # (the same file for both modes: each starts from a copy of the database without it)
    rc, out, err = cli(capfd, "update", "-v", 0, "--db", d, library["imgs"])
    assert rc == 0 and "1 added" in out and "removed %s" % (d / image_search.BIAS_FILE) in out and not (d / image_search.BIAS_FILE).exists()
    rc, out, err = cli(capfd, "search", "--db", d, "--debias", "a red apple")
    assert rc == 1 and image_search.BIAS_FILE in out + err and "debias" in out + err
