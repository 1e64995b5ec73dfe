"""End to end: `image_search search --offset O` over the small database of tests/test_gpu_image_search_file.py (its fixtures are reused)
prints the places O ... O + N - 1 of the ranking `search` prints without it."""
import pytest

from test_gpu_image_search_file import cli, db, library  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def test_offset_prints_the_later_lines(cli, db, capfd):
    hits = lambda out: [ln for ln in out.split("\n") if ln.startswith("  ")]
    rc, five, err = cli(capfd, "search", "--db", db["dir"], "-v", 0, "-n", 5, "a red apple")
    assert rc == 0 and len(hits(five)) == 5, five[-3000:] + err[-3000:]
    rc, out, err = cli(capfd, "search", "--db", db["dir"], "-v", 0, "-n", 3, "--offset", 2, "a red apple")
    assert rc == 0 and hits(out) == hits(five)[2:5], out[-3000:] + err[-3000:]
    assert cli(capfd, "search", "--db", db["dir"], "--offset", 2, "--like", db["paths"][0])[0] == 1
