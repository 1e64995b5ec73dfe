"""Semantic image search over a directory tree: the reference's examples/image-search (`image-search-build` / `image-search`,
build.cpp / search.cpp) on the exact GPU index of this library (`clip_cpp_amd.Index`) instead of usearch's approximate one.

    python -m clip_cpp_amd.image_search build  [-m MODEL] [-v N] [-t N] [--db DIR] [--dtype f16|f32|i8] [--grid G] dir [more dirs]
    python -m clip_cpp_amd.image_search update [-m MODEL] [-v N] [-t N] [--db DIR] dir [more dirs]
    python -m clip_cpp_amd.image_search search [-m MODEL] [-v N] [-t N] [-n N | -d R] [--distinct R] [--in PREFIX]... [--db DIR] <search text or /path/to/query/image>
    python -m clip_cpp_amd.image_search search [-m MODEL] [-v N] [-n N] [--distinct R] [--in PREFIX]... [--db DIR] --like INDEXED/IMAGE/PATH
    python -m clip_cpp_amd.image_search search [-m MODEL] [-v N] [-t N] [-n N] [--in PREFIX]... [--db DIR] [--and TERM]... [--not TERM]... [--not-margin M] <query or --like PATH>
    python -m clip_cpp_amd.image_search dedup  [-m MODEL] [-v N] [--db DIR] [-d R | --max-distance R] [--prune] [--extents]
    python -m clip_cpp_amd.image_search albums [-m MODEL] [-v N] [--db DIR] [-d R | --max-distance R] [--link T] [--min N] [-n COUNT]
    python -m clip_cpp_amd.image_search spread [-m MODEL] [-v N] [--db DIR] -n N [-d R] [--in PREFIX]... [--from INDEXED/IMAGE/PATH]...
    python -m clip_cpp_amd.image_search groups [-m MODEL] [-v N] [--db DIR] -n N [--in PREFIX]... [--min M] [--extents] [--core K]
    python -m clip_cpp_amd.image_search levels [-m MODEL] [-v N] [--db DIR] [--in PREFIX]... [-n ROWS] [--core K]
    python -m clip_cpp_amd.image_search neighbors [-m MODEL] [-v N] [--db DIR] [-n N]
    python -m clip_cpp_amd.image_search label  [-m MODEL] [-v N] [-t N] [--db DIR] [-n N] LABEL [LABEL ...]
    python -m clip_cpp_amd.image_search merge  [-m MODEL] [-v N] --db DIR --from DIR2 [--from DIR3 ...] [-d R]
    python -m clip_cpp_amd.image_search match  [-m MODEL] [-v N] [-t N] [--db DIR] [-n N] [INDEXED/IMAGE/PATH or /path/to/query/image]
    python -m clip_cpp_amd.image_search file   [-m MODEL] [-v N] [-t N] [--db DIR] [-k K] [-n N] [--labels FILE] [--in PREFIX]... IMAGE [IMAGE ...]
    python -m clip_cpp_amd.image_search audit  [-m MODEL] [-v N] [--db DIR] [-k K] [--labels FILE] [--in PREFIX]...

`build` writes DIR/images.index (the CLIPIDX1 file of clip_amd_index_save) and DIR/images.paths (the reference's layout: the model path
on the first line, then one image path per id).  `search` prints the reference's output: "search results:" / "distance path" at
verbosity > 0, then "  %f %s" per hit, nearest first: the -n nearest, or with -d R every indexed image within distance R; with --in PREFIX
(repeatable) only among the images whose path starts with one of the prefixes (the index's subset search: the other rows are not ranked).
`update` brings an existing database in line with the disk without encoding anything twice: every indexed path that no longer exists is
removed from the index (Index.remove + Index.compact), the files under the given dirs that are not indexed yet are encoded and appended,
and both files are rewritten: the survivors in their old order, then the new files in scan order; it prints "main: %d added, %d removed,
%d kept".  `dedup` prints
the groups of near-duplicate images (connected components of the pairs within distance R, computed on the device by Index.components: one
label per image at any number of pairs): "duplicate groups:" at
verbosity > 0, then per group, in order of its lowest id, "  %f %s" per member in id order (the distance to its nearest other member),
groups separated by a blank line, and "main: %d groups, %d images".  `dedup --prune` de-duplicates the database: of every group only the
lowest id stays, the others leave the index (Index.remove + Index.compact) and images.paths, both files are rewritten as `update` rewrites
them, and no image file on disk is touched; it prints the groups at verbosity > 0, then "main: %d removed, %d kept", and rewrites nothing
when there is nothing to remove.
`dedup --extents` and `groups --extents` measure the groups they print (Index.extents over the labels, one call): a group from a chain of
near pairs may be a tight burst of copies or reach far from end to end, and its lowest id is only the first file on disk.  Every group is
printed with its centre first, the member from which the farthest other member is nearest (the lowest id among equals), as
"  %f %f %s": radius (the centre's distance to its farthest member), diameter (the largest distance between two members) and path; the
other members follow in id order as "  %f %s", the distance to their farthest member.  The groups and their order are those without the
flag, and the closing line ends with ", largest diameter %f" (`groups`: "; largest diameter %f").  `dedup --prune --extents` keeps each
group's centre instead of its lowest id.  Without the flag both commands print exactly what they printed before.
`albums` organises the database by content (Index.modes, one call; nothing is encoded): every image points to its nearest image of higher
local density (density = the images within distance R of it, -d as in `dedup`; the parent is looked for within --link T, default R), so
every tree is an album and its root, the most typical image, the cover.  It prints "albums:" at verbosity > 0, then the albums of at
least --min N images (default 2), largest first, equal sizes in order of the cover's id, at most -n COUNT of them: the cover's path on a
line of its own, then "  %f %s" per other member in id order (the distance to its parent), albums separated by a blank line, and
"main: %d albums, %d images".  Among exact copies the lowest id is the cover, the image `dedup --prune` keeps.
`spread -n N` answers "show me N images that between them cover everything in here" (Index.spread, one call; nothing is encoded, nothing
on disk changes): the first indexed image, or the --from images in order, then again and again the image farthest from everything picked
so far, until N are picked or, with -d R, every image is within R of a picked one.  It prints "spread:" at verbosity > 0, then the picks
in order, "%f %s (+K)": the distance at which the image was picked (inf for the first and for --from images; each is the coverage radius
of the picks before it), its path and the number of other images nearer to it than to any other pick; then
"main: %d images, every other image within %f of one of them".  --in PREFIX restricts both the picks and what they cover.  To spread the
results of a search, use the library: Index.search, then Index.spread(n, allow=ids).
`groups -n N` and `levels` need no distance at all: both read the single-linkage tree of the database (Index.linkage, one call: the minimum
spanning tree of the images under the index's distances; nothing is encoded, nothing on disk changes).  `groups -n N` splits the database
into exactly N groups, single images included: the tree without its N - 1 longest links.  It prints "groups:" at verbosity > 0, then the
groups of at least --min M images (default 2) in the format of `dedup`, largest first, equal sizes in order of the lowest id, and
"main: %d groups, %d of them with at least %d images, %d images in those; longest link kept %f, cut at %f": `dedup -d R` finds the same
groups for every R from the first distance up to, not including, the second.  `levels` answers "which -d do I give `dedup`?": the table of
distance against groups from the sorted links of the tree.  It prints "levels:" and "distance groups images largest" at verbosity > 0, then
-n ROWS rows (default 20) evenly spaced over the merges, each moved to the end of its run of equal distances, "  %f %d %d %d": a distance,
the groups of two or more images `dedup` finds at it, the images in them and the size of the largest group; the last row is the distance
at which everything is one group; then "main: %d images, %d levels".  --in PREFIX restricts both commands to the matching images.
`groups --core K` and `levels --core K` read the mutual-reachability tree instead (Index.linkage_core, one call): every distance d(x, y)
is raised to max(d, core(x), core(y)), core being the distance to an image's K-th nearest other image, so an image in a sparse region is
far from everything and a few stray images between two albums no longer chain them into one (the cut at R is DBSCAN* at R with
min_pts = K + 1).  `groups --core K -n N` then asks for exactly N groups of at least --min M images (default 2), at the largest distance
of the tree that gives them (clip_cpp_amd.cut_linkage_sized); smaller groups and single images are left unfiled.  The groups are printed
as without the flag, and the closing line is
"main: %d groups of at least %d images, %d images in those; cut at radius %f, %d images left unfiled"
(--extents adds "; largest diameter %f" as before).  When no distance gives exactly N such groups it prints
"main: -n %d: ..." with the counts that do occur and exits with status 1.  `levels --core K` prints the same table from that tree.
Without --core both commands print exactly what they printed before.
`search --like PATH` asks for "more like this one": the query is the indexed image whose line in images.paths equals PATH as written
(Index.search_ids: its stored row, nothing is decoded or encoded, so a text-only or vision-less model is enough); the image itself is not
listed.  It composes with -n and --in, not with a positional query or -d.
`search --distinct R` folds near-duplicates (bursts, resized copies, re-saved files) into one hit (Index.search_distinct /
Index.search_ids_distinct): walking the ranked list, an image within distance R of an image already listed (the distance of `dedup -d R`)
is dropped, and a listed image that stands for dropped ones gets " (+%d)", their number, behind its path.  The suppression runs over the
pool of the max(64, 8 N) nearest eligible images (at most 1024), not over the whole index.  It works with -n, --in and --like, not with
-d, and not on a database built with --grid.
`search --and TERM` / `--not TERM` (both repeatable, up to 8 terms with the main query) ask compound questions (Index.search_compound):
"a dog" --and "on a beach", --like PATH --and "at night", "a beach" --not "people".  A TERM with an image extension is an image: one that
equals a line of images.paths is that indexed image (its stored row: nothing is decoded or encoded, and it is not listed itself), any
other is a file to load and encode; everything else is text.  The main query and every --and term rank together: --and ranks by the
WORST term, an image's distance column is its largest distance to any of them, so only an image near all of them comes first.  A --not
term keeps only the images that are strictly nearer to all of what is asked for than to that term: its distance must exceed the printed
distance by more than --not-margin M (default 0).  The options go in front of the query; they work with -n, --in and --like, not with -d
or --distinct, and not on a database built with --grid.  `neighbors` prints the k-NN graph (Index.knn_graph, one call):
"neighbours:" at verbosity > 0, then per image, in id order, its path on a line of its own and "  %f %s" per neighbour, the -n (default 5)
nearest other images, nearest first; images separated by a blank line, and "main: %d images, %d neighbours each".
`label` labels the whole database (the reference's zsl example applied to a collection): the labels are encoded as written, in one batch,
into a temporary index of the database's dim and dtype, which is searched once with every stored row of the database
(Index.search_index: no image is decoded or encoded again); "labels:" at verbosity > 0, then per image, in id order, its path on a line of
its own and "  %f %s" (distance, label) for its -n (default 1) nearest labels, nearest first; images separated by a blank line, and
"main: %d images, %d labels each".  `merge` appends the databases given with --from to the one at --db without encoding anything
(Index.append): an image whose path the target already holds is skipped and, with -d R, so is one whose nearest target image is within
R (one Index.search_index per source; listed as "  %f %s ~ %s" at verbosity > 0); it prints "main: %d added, %d already present, %d near
duplicates skipped".  A source built with another model (unless -m is given), dim or dtype is refused before any model is loaded.

`build --grid G` (2 ... 8; 1 is a plain build) indexes regions: every image gives 1 + G * G rows, the whole image and the tiles of a G x G
grid (Clip.encode_image_files(grid=G)), so a small object that hardly moves the embedding of the whole frame still has a row of its own.
images.paths keeps one line per image; DIR/images.regions holds "grid G" and then one line "image x y w h" per index row.  `search` on
such a database ranks images by their best row (Index.search_grouped with group = image): each image is printed once, with its best row's
distance and, when that row is a tile, " [x,y,w,h]" behind the path; a query image is encoded whole; --in selects the rows of the matching
images.  update, merge, dedup, albums, spread, groups, levels, neighbors, label and search --like / -d do not support a database built with --grid yet and say so.

`match` asks a gridded database which other images contain what an image contains: both sides are images made of 1 + G * G rows, and two
images match through their best pair of regions, one from each (query sets: Index.search_ids_sets / Index.search_sets with group = image).
`match PATH` with a path that equals a line of images.paths lists the -n (default 5) nearest OTHER images of that indexed image: its
stored rows are the query set, nothing is decoded or encoded and no tower is needed (the model is loaded only to place the index on its
device), and the image never matches itself through its own rows.  `match FILE` with any other image file encodes it with
Clip.encode_image_files(grid=G), G from images.regions, into one set of 1 + G * G vectors.  Each hit is "  %f %s" (distance, path),
then " [x,y,w,h]" when the stored row of the best pair is a tile (the suffix of `search`), then " <- [x,y,w,h]" when the query row is a
tile of the query image.  `match` without a path prints every image's matches (Index.knn_graph_grouped, one call) in the output shape of
`neighbors`: "matches:" at verbosity > 0, per image its path and its hits, images separated by a blank line, and "main: %d images, %d
matches each".  On a plain database `match` stops before any model is loaded and points to `search --like` / `neighbors`.

`file` and `audit` use the labels a library already carries, its folders, through a k-nearest-neighbour vote over the stored rows
(Index.vote / Index.vote_ids / Index.vote_graph): an image's class is the directory part of its line in images.paths, as written, or with
--labels FILE (lines "label<TAB>path") the label listed for its path; an image the file does not list is unlabelled: it may be asked about
but never votes, and a path in the file that is not indexed is an error that names it.  --in PREFIX lets only the matching images vote.
`file IMAGE...` answers "into which of my folders does this picture go?": an IMAGE that equals a line of images.paths is that stored row
(nothing is decoded, and the row itself does not vote), any other is a file to load and encode.  The -k K (default 10) nearest voters
vote; it prints "filing:" at verbosity > 0, then per image its path on a line of its own and, for each of the -n N (default 3) best
classes, "  %d/%d %f %s ~ %s": votes, voters counted, the distance of the class's nearest member, the class and that member's path; images
are separated by a blank line, and the last line is "main: %d images, %d voters each".  `audit` is the leave-one-out twin, "which
pictures lie in the wrong folder?" (one Index.vote_graph call; no image is decoded or encoded): "misfiled:" at verbosity > 0, then for
every labelled image whose winning class is not its own, in id order, "  %d/%d %f %s -> %s ~ %s": the winner's votes, voters counted, the
distance of the winner's nearest member, the image's path, the winning class and that member's path; then
"main: %d labelled images, %d filed against their neighbours, %d with no voter".  Neither supports a database built with --grid.
"""
import ctypes as C
import os
import struct
import sys

import numpy as np

IMAGE_EXTENSIONS = (".jpg", ".JPG", ".jpeg", ".JPEG", ".gif", ".GIF", ".png", ".PNG")
INDEX_FILE = "images.index"
PATHS_FILE = "images.paths"
REGIONS_FILE = "images.regions"
MAX_GRID = 8
BATCH = 64          # images decoded and encoded per call
MAX_K = 1024
DEDUP_RADIUS = 0.05
MAX_TERMS = 8       # terms of a compound search: the main query, every --and and every --not
LEVEL_ROWS = 20     # rows of the `levels` table
MAX_CORE = 1024     # --core K of `groups` and `levels`: the k of Index.linkage_core


EXTENTS_HELP = ("  --extents: measure every group (Index.extents): its centre, the image from which the farthest other member is nearest, comes"
                " first as `radius diameter path` (the distance from the centre to its farthest member, and the largest distance between two"
                " members: a tight burst of copies has a small diameter, a chain of near pairs a large one); the other members follow with"
                " the distance to their farthest member. The last line adds the largest diameter found.%s")


def is_image_file_extension(path):
    """The reference's is_image_file_extension (examples/common-clip.cpp): the text after the last '.' is one of eight spellings."""
    pos = path.rfind(".")
    return pos >= 0 and path[pos:] in IMAGE_EXTENSIONS


def classify_query(args):
    """(image_path, search_text) from the positional arguments the way the reference's parser reads them: a last argument with an image
    extension is an image query; otherwise the arguments from the first one on are joined with spaces into the search text."""
    if not args:
        return "", ""
    if len(args) == 1 and is_image_file_extension(args[0]):
        return args[0], ""
    return "", " ".join(args)


def _err(msg):
    print(msg, file=sys.stderr, flush=True)


def _parse(argv, build, dedup=False, update=False, neighbors=False, label=False, merge=False, match=False, albums=False, spread=False,
           groups=False, levels=False):
    """Reference-style option parsing (examples/image-search/{build,search}.cpp my_app_params_parse); `dedup`, `albums`, `spread`, `neighbors`
    and `merge` take no positional arguments; `spread` needs -n; `update` takes build's directories, but neither a default model nor --dtype (both come from the database);
    `label` takes the labels; `merge` needs --from at least once; `match` takes at most one image path; `groups` and `levels` take no
    positional arguments either, `groups` needs -n."""
    p = dict(threads=4, verbose=1, db=".", dtype="f16", results=1 if label else 5, max_distance=DEDUP_RADIUS if dedup or albums else None,
             model="../models/ggml-model-f16.bin" if build else "", rest=[], like=None)
    p["in"] = []
    if groups or levels:
        p["core"] = None                                   # --core K: the mutual-reachability tree
    if merge or spread:
        p["from"] = []
    if spread:
        p.update(results=None)                             # -n has no default: it is the question
    if albums:
        p.update(results=None, link=None, min_size=2)      # every album; link = the radius
    if groups:
        p.update(results=None, min_size=2)                 # -n has no default: it is the question
    if levels:
        p.update(results=LEVEL_ROWS)
    tree = groups or levels
    search = not (build or dedup or update or neighbors or label or merge or match or albums or spread or tree)
    seen = set()
    i = 0
    while i < len(argv):
        a = argv[i]
        takes = {"-m": "model", "--model": "model", "-v": "verbose", "--verbose": "verbose", "--db": "db"}
        if not (dedup or neighbors or merge or albums or spread or tree):
            takes.update({"-t": "threads", "--threads": "threads"})
        if build:
            takes["--dtype"] = "dtype"
            takes["--grid"] = "grid"
        elif neighbors or label or match:
            takes.update({"-n": "results", "--results": "results"})
        elif tree:
            takes.update({"-n": "results", "--results": "results", "--in": "in", "--core": "core"})
            if groups:
                takes["--min"] = "min_size"
        elif merge:
            takes.update({"-d": "max_distance", "--max-distance": "max_distance", "--from": "from"})
        elif spread:
            takes.update({"-d": "max_distance", "--max-distance": "max_distance", "-n": "results", "--results": "results", "--in": "in",
                          "--from": "from"})
        elif albums:
            takes.update({"-d": "max_distance", "--max-distance": "max_distance", "--link": "link", "--min": "min_size", "-n": "results",
                          "--results": "results"})
        elif not update:
            takes.update({"-d": "max_distance", "--max-distance": "max_distance"})
            if not dedup:
                takes.update({"-n": "results", "--results": "results"})
        if search:
            takes.update({"--in": "in", "--like": "like", "--distinct": "distinct", "--and": "and", "--not": "not", "--not-margin": "not_margin"})
        if a in takes:
            i += 1
            if i >= len(argv):
                return None
            key = takes[a]
            if key == "like" and "like" in seen:
                print("main: --like takes one indexed image: it cannot be given twice")
                return None
            seen.add(key)
            if key in ("in", "from", "and", "not"):
                p.setdefault(key, []).append(argv[i])
                i += 1
                continue
            try:
                p[key] = int(argv[i]) if key in ("threads", "verbose", "results", "grid", "min_size", "core") else float(argv[i]) if key in ("max_distance", "distinct", "not_margin", "link") else argv[i]
            except ValueError:
                return None
            if key in ("max_distance", "distinct", "not_margin", "link") and p[key] != p[key]:      # NaN
                return None
            if key == "grid" and not 1 <= p[key] <= MAX_GRID:
                print("main: --grid takes 1 ... %d (1: whole images only), not %d" % (MAX_GRID, p[key]))
                return None
        elif dedup and a == "--prune":
            p["prune"] = True
        elif (dedup or groups) and a == "--extents":
            p["extents"] = True
        elif a in ("-h", "--help"):
            _help(build, p, dedup, update, neighbors, label, merge, match, albums, spread, groups, levels)
            sys.exit(0)
        elif a.startswith("-"):
            print("main: unrecognized argument: %s" % a)
            return None
        elif dedup or neighbors or merge or albums or spread or tree:
            print("main: unexpected argument: %s" % a)
            return None
        elif build or update or label or match:
            p["rest"].append(a)
        else:
            p["rest"] = argv[i:]     # the query: everything from here on
            break
        i += 1
    if p["like"] is not None:
        if p["rest"] or "max_distance" in seen:
            print("main: --like cannot be combined with a query or with -d: it lists the -n nearest images of an indexed one")
            return None
    elif (not p["rest"] and not (dedup or neighbors or merge or match or albums or spread or tree)) or (build and p["dtype"] not in ("f16", "f32", "i8")):
        return None
    if merge and not p["from"]:
        return None
    if spread:
        if p["results"] is None:
            return None
        if len(set(p["from"])) != len(p["from"]):
            print("main: --from names the first images to take: each can be given once")
            return None
        if p["results"] < max(1, len(p["from"])):
            print("main: -n %d: spread picks at least one image and at least the %d given with --from" % (p["results"], len(p["from"])))
            return None
    if groups:
        if p["results"] is None:
            return None
        if p["results"] < 1:
            print("main: -n %d: groups makes at least one group" % p["results"])
            return None
    if (groups or levels) and p["core"] is not None and not 0 <= p["core"] <= MAX_CORE:
        print("main: --core takes 0 ... %d (0: the single-linkage tree), not %d" % (MAX_CORE, p["core"]))
        return None
    if levels and p["results"] < 1:
        print("main: -n %d: levels prints at least one row" % p["results"])
        return None
    if match and len(p["rest"]) > 1:
        print("main: match takes one image path, or none for every indexed image")
        return None
    if seen & {"and", "not", "not_margin"}:
        if "max_distance" in seen or "distinct" in seen:
            print("main: --and / --not cannot be combined with -d or --distinct: they rank the -n nearest images by their worst term")
            return None
        if "not_margin" in seen and "not" not in seen:
            print("main: --not-margin is the margin of the --not terms: it needs at least one --not")
            return None
        if 1 + len(p.get("and", [])) + len(p.get("not", [])) > MAX_TERMS:
            print("main: a compound search takes at most %d terms (the query, every --and and every --not), not %d"
                  % (MAX_TERMS, 1 + len(p.get("and", [])) + len(p.get("not", []))))
            return None
    if {"distinct", "max_distance"} <= seen:
        print("main: --distinct and -d cannot be combined: --distinct R thins the -n nearest, -d R prints every image within R")
        return None
    if {"results", "max_distance"} <= seen and not (albums or spread):     # (albums: -n counts albums, -d is the density radius; spread: both end it)
        print("main: -n and -d cannot be combined: -n N prints the N nearest, -d R every image within R")
        return None
    return p


def _help(build, p, dedup=False, update=False, neighbors=False, label=False, merge=False, match=False, albums=False, spread=False,
          groups=False, levels=False):
    radius = ("  -d R, --max-distance R: %s within cosine distance R (<= R). Default: %s. %g is a starting point for embeddings of near-identical"
              " images, not a tuned value: check a few groups of your collection and adjust R")
    if groups or levels:
        if groups:
            print("Usage: python -m clip_cpp_amd.image_search groups [options] -n N")
            print("\nSplits the images of an index built by `build` into exactly N groups: the single-linkage tree of the index (its minimum")
            print("spanning tree) without its N - 1 longest links. No distance has to be guessed. Nothing is encoded, nothing on disk changes.")
            print("Groups are printed as `dedup` prints them, the largest first; the last line states the distance at which the tree was cut.")
        else:
            print("Usage: python -m clip_cpp_amd.image_search levels [options]")
            print("\nPrints the table of distance against groups for an index built by `build`: what `dedup -d R` would find at each R, from one")
            print("pass over the single-linkage tree of the index. Each row: a distance, the groups of two or more images at it, the images in")
            print("them and the size of the largest group. Nothing is encoded, nothing on disk changes.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default (loaded only to place the index on its device).")
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        if groups:
            print("  -n N, --results N: make exactly N groups, single images included. Required")
            print("  --min M: print only the groups of at least M images. Default: 2 (1: single images too)")
            print("  --core K: read the mutual-reachability tree (distances raised to the distance of either image's K-th nearest other image), so a")
            print("    few stray images between two groups do not chain them together. -n N then asks for exactly N groups of at least --min M images;")
            print("    smaller groups and single images are left unfiled. Exits with status 1 when no distance gives exactly N such groups")
        else:
            print("  -n ROWS, --results ROWS: rows of the table, evenly spaced over the merges of the tree. Default: %d" % LEVEL_ROWS)
            print("  --core K: the table of the mutual-reachability tree (see `groups --core K`): what `groups --core K` finds at each distance")
        print("  --in <prefix>: only images whose indexed path starts with <prefix> take part; may be repeated")
        if groups:
            print(EXTENTS_HELP % "")
    elif spread:
        print("Usage: python -m clip_cpp_amd.image_search spread [options] -n N")
        print("\nPicks N images of an index built by `build` that between them cover the collection: the first indexed image (or the --from")
        print("images), then again and again the image farthest from everything picked so far. Nothing is encoded, nothing on disk changes.")
        print("Each line is the distance at which the image was picked (how far the farthest image was from the picks before it), its path and")
        print("the number of other images that are nearer to it than to any other pick.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default (loaded only to place the index on its device).")
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print("  -n N, --results N: pick N images (fewer when there are fewer, or when -d ends it). Required")
        print("  -d R, --max-distance R: stop once every image is within cosine distance R (<= R) of a picked one. Default: never")
        print("  --in <prefix>: only images whose indexed path starts with <prefix> are picked from and covered; may be repeated")
        print("  --from <indexed/image/path>: start from this image, as written in %s; may be repeated: they are taken first, in order."
              " Default: the first indexed image" % PATHS_FILE)
    elif albums:
        print("Usage: python -m clip_cpp_amd.image_search albums [options]")
        print("\nGroups the images of an index built by `build` into albums, each with a cover: every image points to its nearest image of higher")
        print("local density, every tree of that forest is an album and its root, the most typical image, the cover. Nothing is encoded.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default (loaded only to place the index on its device).")
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print(radius % ("an image's density is the number of images", DEDUP_RADIUS, DEDUP_RADIUS))
        print("  --link T: an image joins the album of its nearest image of higher density (equal density: lower id) within cosine distance T"
              " (<= T). Default: R. A larger T gives fewer, larger albums")
        print("  --min N: print only the albums of at least N images. Default: 2 (1: single images too)")
        print("  -n COUNT, --results COUNT: print at most COUNT albums, the largest. Default: all")
    elif match:
        print("Usage: python -m clip_cpp_amd.image_search match [options] [indexed/image/path or /path/to/query/image]")
        print("\nOn a database built with `build --grid G`: the other images that contain what an image contains. Two images match through")
        print("their best pair of regions, one from each. A path that equals a line of %s is an indexed image (nothing is decoded or" % PATHS_FILE)
        print("encoded); any other path is an image file, encoded as its 1 + G*G regions; without a path, every indexed image's matches.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default (an indexed image needs no tower: the"
              " model is loaded only to place the index on its device; an image file needs the vision encoder).")
        print("  -t N, --threads N: Number of host threads that read and decode a query image file. Default: %d" % p["threads"])
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s, %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, REGIONS_FILE, p["db"]))
        print("  -n N, --results N: Number of matching images per image (at most %d). Default: %d" % (MAX_K, p["results"]))
    elif label:
        print("Usage: python -m clip_cpp_amd.image_search label [options] LABEL [LABEL ...]")
        print("\nPrints, for every image of an index built by `build`, the labels that fit it best. The labels are encoded as written (no prompt")
        print("template); no image is decoded or encoded again.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default. The model needs a text encoder.")
        print("  -t N, --threads N: Number of threads to use for inference. Default: %d" % p["threads"])
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print("  -n N, --results N: Number of labels per image, nearest first (at most %d). Default: %d" % (MAX_K, p["results"]))
    elif merge:
        print("Usage: python -m clip_cpp_amd.image_search merge [options] --db <dir> --from <dir2> [--from <dir3> ...]")
        print("\nAppends the databases given with --from to the one at --db without encoding anything twice. Images whose path the target")
        print("already holds are skipped. Every database must have been built with the same model, dim and dtype.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model (loaded only to place the indexes on its device); the model lines of the"
              " databases are then not compared, and the given path is the one stored in the merged %s." % PATHS_FILE)
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: the target: directory holding %s and %s; both are written under temporary names and renamed into place."
              " Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print("  --from <dir>: a source database to append; may be repeated. Sources are not changed")
        print("  -d R, --max-distance R: also skip a source image whose nearest target image is within cosine distance R (<= R): an import"
              " without near duplicates. Default: off. %g is a starting point for near-identical images, not a tuned value" % DEDUP_RADIUS)
    elif neighbors:
        print("Usage: python -m clip_cpp_amd.image_search neighbors [options]")
        print("\nPrints, for every image of an index built by `build`, its nearest other images (the k-NN graph of the index).")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default (loaded only to place the index on its device).")
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print("  -n N, --results N: Number of neighbours per image (at most %d). Default: %d" % (MAX_K, p["results"]))
    elif dedup:
        print("Usage: python -m clip_cpp_amd.image_search dedup [options]")
        print("\nPrints the groups of near-duplicate images of an index built by `build` (connected components of the image pairs within R),")
        print("or with --prune removes all but one image of every group from the database.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default (loaded only to place the index on its device).")
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print(radius % ("pair images", DEDUP_RADIUS, DEDUP_RADIUS))
        print("  --prune: de-duplicate the database: of every group only the first image (the lowest id) stays in %s and %s, both"
              " rewritten under temporary names and renamed into place; image files on disk are never touched. Prints the groups at"
              " verbosity > 0, then the number of images removed and kept" % (INDEX_FILE, PATHS_FILE))
        print(EXTENTS_HELP % " With --prune the centre is the image that stays, not the lowest id.")
    elif update:
        print("Usage: python -m clip_cpp_amd.image_search update [options] dir/with/pictures [more/dirs]")
        print("\nBrings a database made by `build` in line with the disk: indexed paths that no longer exist are removed, image files under the")
        print("given dirs that are not indexed yet are encoded and appended, nothing already indexed is encoded again.")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default. When the database is rewritten, the"
              " given path replaces the one stored on the first line of images.paths: later commands load this model.")
        print("  -t N, --threads N: Number of host threads that read and decode the image files. Default: %d" % p["threads"])
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory holding %s and %s; both are written under temporary names and renamed into place. Default: %s"
              % (INDEX_FILE, PATHS_FILE, p["db"]))
    elif build:
        print("Usage: python -m clip_cpp_amd.image_search build [options] dir/with/pictures [more/dirs]")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: path to model. Default: %s" % p["model"])
        print("  -t N, --threads N: Number of host threads that read and decode the image files. Default: %d" % p["threads"])
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  --db <dir>: directory that receives %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
        print("  --dtype f16|f32|i8: stored precision of the index (i8: int8 rows, half of f16's memory). Default: %s" % p["dtype"])
        print("  --grid G: index regions as well: every image gives 1 + G*G rows, the whole image and the tiles of a G x G grid, and `search`"
              " ranks images by their best row (2 ... %d; update, merge, dedup, albums, neighbors, label and search --like / -d do not support such"
              " a database yet). Default: 1, whole images only" % MAX_GRID)
    else:
        print("Usage: python -m clip_cpp_amd.image_search search [options] <search string or /path/to/query/image>")
        print("       python -m clip_cpp_amd.image_search search [options] --like <indexed/image/path>")
        print("\nOptions:")
        print("  -h, --help: Show this message and exit")
        print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default.")
        print("  -t N, --threads N: Number of threads to use for inference. Default: %d" % p["threads"])
        print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
        print("  -n N, --results N: Number of results to display. Default: %d" % p["results"])
        print("  -d R, --max-distance R: display every indexed image within cosine distance R (<= R), nearest first, instead of the -n nearest (not with -n)")
        print("  --in <prefix>: only images whose indexed path starts with <prefix> are eligible (one directory, one album); may be repeated:"
              " a path matching any prefix is eligible. Works with -n and with -d")
        print("  --like <path>: more like this one: the query is the indexed image whose line in %s equals <path> as written; nothing is"
              " decoded or encoded and the image itself is not listed. Works with -n and --in, not with a query or -d" % PATHS_FILE)
        print("  --distinct R: fold near-duplicates into one hit: walking the ranked list, an image within cosine distance R (<= R, the distance"
              " of `dedup -d R`) of an image already listed is dropped, and a listed image is followed by (+N), the number of images dropped"
              " for it. Suppression runs over the max(64, 8 N) nearest eligible images (at most %d), not the whole index. Works with -n, --in"
              " and --like, not with -d" % MAX_K)
        print("  --and <term>: a compound search: rank by the WORST term, an image's distance is its largest distance to the query and to every"
              " --and term, so only an image near all of them comes first; may be repeated. A term with an image extension is an image: one"
              " that equals a line of %s is that indexed image (its stored row; it is not listed itself), any other is a file to load and"
              " encode; everything else is text. Works with -n, --in and --like, not with -d or --distinct; options go in front of the query"
              % PATHS_FILE)
        print("  --not <term>: only images strictly nearer to the query (and every --and term) than to this term; may be repeated. At most %d"
              " terms in all: the query, every --and and every --not" % MAX_TERMS)
        print("  --not-margin M: the distance to a --not term must exceed the printed distance by more than M. Default: 0")
        print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))


def image_files(base_dir):
    """Every file under base_dir (recursively, in sorted order) whose extension passes is_image_file_extension."""
    out = []
    for root, dirs, files in os.walk(base_dir):
        dirs.sort()
        for name in sorted(files):
            if is_image_file_extension(name):
                out.append(os.path.join(root, name))
    return out


def _encode_batch(clip, L, imgs):
    """embeddings [n, proj] of decoded clip_image_u8 structs through clip_amd_image_batch_encode_u8, normalised"""
    import clip_cpp_amd
    arr = (clip_cpp_amd.ClipImageU8 * len(imgs))(*[im.contents for im in imgs])
    out = np.empty((len(imgs), clip.vision_config["projection_dim"]), dtype=np.float32)
    if not L.clip_amd_image_batch_encode_u8(clip.ctx, arr, len(imgs), out.ctypes.data_as(C.POINTER(C.c_float)), True):
        raise RuntimeError("clip_amd_image_batch_encode_u8 failed (see stderr)")
    return out


def build(argv):
    import clip_cpp_amd
    p = _parse(argv, build=True)
    if p is None:
        _help(True, dict(threads=4, verbose=1, db=".", dtype="f16", model="../models/ggml-model-f16.bin"))
        return 1
    L = clip_cpp_amd.lib()
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])
    except RuntimeError:
        print("main: Unable  to load model from %s" % p["model"])
        return 1
    if clip.vision_config["n_layer"] <= 0:
        _err("main: the model at %s has no vision encoder: an image index needs a vision or two-tower model" % p["model"])
        return 1
    index = clip_cpp_amd.Index(clip, clip.vision_config["projection_dim"], dtype=p["dtype"])
    paths = []
    p.setdefault("grid", 1)                        # (the key exists only when --grid was given)
    regions = [] if p["grid"] > 1 else None
    _encode_dirs(clip, L, index, p, paths, regions=regions)
    os.makedirs(p["db"], exist_ok=True)
    _write_db(p, index, paths, regions)
    index.close()
    clip.close()
    print("main: %d images processed and indexed" % len(paths), flush=True)
    return 0


def _write_db(p, index, paths, regions=None):
    """Both files under temporary names first, then renamed into place one after the other: an interruption while they are written
    leaves the old database as it was.  regions (a build with --grid): the (image, x, y, w, h) of every index row, written the same way
    as the third file; without them a regions file left by an earlier gridded build of the same directory goes away."""
    index_file, paths_file = os.path.join(p["db"], INDEX_FILE), os.path.join(p["db"], PATHS_FILE)
    regions_file = os.path.join(p["db"], REGIONS_FILE)
    index.save(index_file + ".tmp")
    with open(paths_file + ".tmp", "w") as f:
        f.write(p["model"] + "\n")
        for path in paths:
            f.write(path + "\n")
    if regions is not None:
        with open(regions_file + ".tmp", "w") as f:
            f.write("grid %d\n" % p["grid"])
            for row in regions:
                f.write("%d %d %d %d %d\n" % tuple(row))
    os.replace(index_file + ".tmp", index_file)
    os.replace(paths_file + ".tmp", paths_file)
    if regions is not None:
        os.replace(regions_file + ".tmp", regions_file)
    elif os.path.exists(regions_file):
        os.remove(regions_file)


def read_regions(db):
    """(grid, int array [rows, 5] = image, x, y, w, h) of db/images.regions; None when the database has none (a plain build); ValueError
    when the file is not a regions file as `build --grid` writes it: the rows of an image together, images in ascending order, 1 + G * G
    rows each (`search` takes an image's first row for the whole image and the others for tiles)."""
    regions_file = os.path.join(db, REGIONS_FILE)
    if not os.path.exists(regions_file):
        return None
    with open(regions_file) as f:
        lines = f.read().split("\n")
    head = lines[0].split()
    if len(head) != 2 or head[0] != "grid":
        raise ValueError("'%s' does not start with 'grid G'" % regions_file)
    rows = [[int(v) for v in line.split()] for line in lines[1:] if line]
    if any(len(r) != 5 for r in rows):
        raise ValueError("'%s' holds a line that is not 'image x y w h'" % regions_file)
    grid, rows = int(head[1]), np.array(rows, dtype=np.int64).reshape(-1, 5)
    per = 1 + grid * grid
    if not 2 <= grid <= MAX_GRID or len(rows) % per or not np.array_equal(rows[:, 0], np.repeat(rows[::per, 0], per)) or \
            (len(rows) > per and np.any(np.diff(rows[::per, 0]) <= 0)):
        raise ValueError("'%s' does not hold %s rows per image, each image's rows together and the images in ascending order"
                         % (regions_file, "1 + G * G" if not 2 <= grid <= MAX_GRID else per))
    return grid, rows


def _refuse_gridded(db, command):
    """True, with the message printed, when the database in db was built with --grid: `command` does not handle regions"""
    if not os.path.exists(os.path.join(db, REGIONS_FILE)):
        return False
    _err("main: the database in '%s' was built with --grid (it holds %s): `%s` does not support such a database yet"
         % (db, REGIONS_FILE, command))
    return True


def _encode_dirs(clip, L, index, p, paths, scans=None, regions=None):
    """Decode and encode the image files of the directories p["rest"] in batches and append them to `index` and `paths`.  scans: the
    [(dir, files)] to take when the caller has scanned already (`update`), else every file found under each dir.
    The files of all directories form one list that goes through Clip.encode_image_files in windows of BATCH loadable images:
    p["threads"] host threads read and decode (the GPU does the JPEG pixel work unless CLIP_AMD_JPEG_DEVICE=0), and every encoder call
    sees BATCH consecutive loadable images, across directory boundaries too.  The directories are scanned first and each is announced
    when its first file is reported, so the lines come out in the order of a file-by-file pass; the list is prepared for the library
    once (Clip.ImageFileList), each call starts where the last one stopped and no file is decoded twice.
    regions (a list, build --grid): every image is encoded as the 1 + G * G rows of Clip.encode_image_files(grid=p["grid"]) and the list
    receives (image id, x, y, w, h) per row."""
    stream, heads = [], []                            # heads: (index of the directory's first file in stream, dir, files, scanned here)
    for base, files in scans if scans is not None else [(base, None) for base in p["rest"]]:
        heads.append((len(stream), base, image_files(base) if files is None else files, files is None))
        stream.extend(heads[-1][2])

    def announce(upto):
        while heads and heads[0][0] <= upto:
            _, base, files, here = heads.pop(0)
            if here:
                print("main: starting base dir scan of '%s'" % base, flush=True)
            print("\nmain: processing %d files in '%s'" % (len(files), base), flush=True)

    prepared, pos = clip.ImageFileList(stream), 0
    while pos < len(stream):
        if regions is None:
            vecs, ok, consumed = clip.encode_image_files(prepared, normalize=True, n_threads=p["threads"], max_images=BATCH, start=pos)
        else:
            vecs, ok, consumed, boxes = clip.encode_image_files(prepared, normalize=True, n_threads=p["threads"], max_images=BATCH, start=pos,
                                                                grid=p["grid"])
        if consumed <= 0:
            break
        window = stream[pos:pos + consumed]
        for i, (path, good) in enumerate(zip(window, ok)):
            announce(pos + i)
            if p["verbose"] >= 2:
                print("main: found image file '%s'" % path, flush=True)
            if not good:
                _err("main: failed to load image from '%s'" % path)      # (no slot: the failed file gets no id and no line in images.paths)
        pos += consumed
        loaded = [path for path, good in zip(window, ok) if good]
        if loaded:
            index.add(vecs)
            if regions is not None:
                per = len(boxes) // len(loaded)
                for r, box in enumerate(boxes.tolist()):
                    regions.append([len(paths) + r // per] + box)
            paths.extend(loaded)
            if p["verbose"] == 1:
                print(".", end="", flush=True)
    announce(len(stream))


def reconcile(old_paths, found, exists=os.path.exists):
    """What `update` does to a database: (kept, removed, to_add).  kept: the ids of old_paths that still exist, ascending; removed: the ids
    that do not; to_add: the files of `found` (scan order) that are not indexed, each once."""
    kept = [i for i, path in enumerate(old_paths) if exists(path)]
    kept_set = set(kept)
    removed = [i for i in range(len(old_paths)) if i not in kept_set]
    known = set(old_paths[i] for i in kept)
    to_add = []
    for path in found:
        if path not in known:
            known.add(path)
            to_add.append(path)
    return kept, removed, to_add


def update(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, update=True)
    if p is None:
        _help(False, dict(threads=4, verbose=1, db="."), update=True)
        return 1
    if _refuse_gridded(p["db"], "update"):
        return 1
    old_paths = _read_db(p)
    if old_paths is None:
        return 1
    scans = []
    for base in p["rest"]:                          # every directory is scanned once
        print("main: starting base dir scan of '%s'" % base, flush=True)
        scans.append((base, image_files(base)))
    kept, removed, to_add = reconcile(old_paths, [f for _, files in scans for f in files])
    L = clip_cpp_amd.lib()
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    if to_add and clip.vision_config["n_layer"] <= 0:
        _err("main: the model at %s has no vision encoder: an image index needs a vision or two-tower model" % p["model"])
        return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    if to_add and index.dim != clip.vision_config["projection_dim"]:
        _err("main: the index holds %d-dimensional embeddings, the model makes %d" % (index.dim, clip.vision_config["projection_dim"]))
        return 1
    paths = [old_paths[i] for i in kept]
    if removed:
        index.remove(removed)
        index.compact()
    n_kept = len(paths)
    if to_add:
        todo = set(to_add)
        for i, (base, files) in enumerate(scans):   # each new file under the first directory that holds it
            scans[i] = (base, [f for f in files if f in todo])
            todo -= set(scans[i][1])
        _encode_dirs(clip, L, index, p, paths, scans)
    if removed or len(paths) > n_kept:
        _write_db(p, index, paths)
    index.close()
    clip.close()
    print("main: %d added, %d removed, %d kept" % (len(paths) - n_kept, len(removed), n_kept), flush=True)
    return 0


def read_index_header(path):
    """(version, dim, dtype, n) of a CLIPIDX1 file, or None when it is not one."""
    try:
        with open(path, "rb") as f:
            h = f.read(28)
    except OSError:
        return None
    if len(h) != 28 or h[:8] != b"CLIPIDX1":
        return None
    return struct.unpack("<IIIQ", h[8:])


def _read_paths(db):
    """(model line, image paths) of db/images.paths; ("", []) when the file is missing or empty."""
    paths_file = os.path.join(db, PATHS_FILE)
    lines = []
    if os.path.exists(paths_file):
        with open(paths_file) as f:
            lines = f.read().split("\n")
    model_line = lines[0] if lines else ""
    image_paths = []
    for line in lines[1:]:
        if not line:
            break
        image_paths.append(line)
    return model_line, image_paths


def _read_db(p, regions=None):
    """The image paths of DIR/images.paths after the database checks `search` and `dedup` share (the model path from its first line unless
    -m gave one); None, with the message printed, when a check fails.  regions (read_regions, a gridded database): the index holds one
    row per region, each naming one of the paths."""
    model_line, image_paths = _read_paths(p["db"])
    if not p["model"]:
        p["model"] = model_line
    else:
        print("main: using alternative model from %s. Make sure you use the same model you used for indexing, or the embeddings wont work."
              % p["model"])
    if not p["model"]:
        print("main: Unable to load model from %s" % p["model"])
        _err("main: no database in '%s' (%s is missing or empty): run `python -m clip_cpp_amd.image_search build` first" % (p["db"], PATHS_FILE))
        return None
    hdr = read_index_header(os.path.join(p["db"], INDEX_FILE))
    if hdr is None:
        _err("main: '%s' is missing or not an index file" % os.path.join(p["db"], INDEX_FILE))
        return None
    if regions is not None:
        rows = regions[1]
        if hdr[3] != len(rows) or (len(rows) and (rows[:, 0].min() < 0 or rows[:, 0].max() >= len(image_paths))):
            print("main: index files size missmatch")
            return None
        return image_paths
    if hdr[3] != len(image_paths):
        print("main: index files size missmatch")
        return None
    return image_paths


def search(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False)
    if p is None:
        _help(False, dict(threads=4, verbose=1, db=".", results=5))
        return 1
    img_path, text = classify_query(p["rest"])
    if p.get("distinct") is not None and _refuse_gridded(p["db"], "search --distinct"):
        return 1
    compound = bool(p.get("and") or p.get("not"))
    if compound and _refuse_gridded(p["db"], "search --and / --not"):
        return 1
    if (p["like"] is not None or p["max_distance"] is not None) and _refuse_gridded(p["db"], "search --like" if p["like"] is not None else "search -d"):
        return 1
    try:
        regions = read_regions(p["db"])
    except ValueError as e:
        _err("main: %s" % e)
        return 1
    image_paths = _read_db(p, regions)
    if image_paths is None:
        return 1
    like_id = None
    if p["like"] is not None:
        if p["like"] not in image_paths:
            _err("main: '%s' is not in the database (paths are compared as written in %s)" % (p["like"], PATHS_FILE))
            return 1
        like_id = image_paths.index(p["like"])
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    if compound:
        return _search_compound(clip_cpp_amd, clip, p, image_paths, like_id, img_path, text)
    vec = None
    if like_id is not None:
        pass                                       # the query is a stored row: no tower is needed
    elif img_path:
        if clip.vision_config["n_layer"] <= 0:
            _err("main: the model at %s has no vision encoder: image queries need a vision or two-tower model" % p["model"])
            return 1
        L = clip_cpp_amd.lib()
        im = L.clip_image_u8_make()
        try:
            if not L.clip_image_load_from_file(os.fsencode(img_path), im):
                _err("main: failed to load image from '%s'" % img_path)
                return 1
            vec = _encode_batch(clip, L, [im])[0]
        finally:
            L.clip_image_u8_free(im)
    else:
        if clip.text_config["n_layer"] <= 0:
            _err("main: the model at %s has no text encoder: text queries need a two-tower model" % p["model"])
            return 1
        vec = np.asarray(clip.encode_text(clip.tokenize(text), n_threads=p["threads"], normalize=True), dtype=np.float32)
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    if vec is not None and index.dim != vec.size:
        _err("main: the index holds %d-dimensional embeddings, the model makes %d" % (index.dim, vec.size))
        return 1
    allow = None
    if p["in"]:                                    # the index ranks only these rows: no host-side filtering of a longer list
        allow = np.array([path.startswith(tuple(p["in"])) for path in image_paths], dtype=np.bool_)
    boxes = {}
    more = {}                                      # --distinct: id -> the number of images folded into that hit
    if regions is not None:                        # images ranked by their best row: group = image, each image once
        rows = regions[1]
        groups = rows[:, 0]
        k = max(1, min(p["results"], MAX_K))
        dist, ids = index.search_grouped(vec[None, :], k, groups, allow=None if allow is None else allow[groups])
        whole = np.ones(len(rows), dtype=np.bool_)
        whole[1:] = groups[1:] != groups[:-1]      # an image's first row is the whole image, the tiles follow
        hits = []
        for d, r in zip(dist[0], ids[0]):
            if r >= 0 and p["results"] > 0:
                hits.append((d, int(groups[r])))
                if not whole[r]:
                    boxes[int(groups[r])] = " [%d,%d,%d,%d]" % tuple(rows[r, 1:])
    elif p["max_distance"] is not None:
        _, dist, ids = index.range_search(vec[None, :], p["max_distance"], allow=allow)
        hits = list(zip(dist, ids))
    elif p.get("distinct") is not None:
        k = max(1, min(p["results"], MAX_K))
        if len(index) == 0:                        # (the library refuses an empty index)
            dist, ids, counts = np.zeros((1, 0), np.float32), np.zeros((1, 0), np.int64), np.zeros((1, 0), np.int32)
        elif like_id is not None:
            dist, ids, counts = index.search_ids_distinct([like_id], k, p["distinct"], allow=allow)
        else:
            dist, ids, counts = index.search_distinct(vec[None, :], k, p["distinct"], allow=allow)
        hits = [(d, i) for d, i in zip(dist[0], ids[0]) if i >= 0 and p["results"] > 0]
        more = {int(i): int(c) for i, c in zip(ids[0], counts[0]) if i >= 0 and c > 0}
    else:
        k = max(1, min(p["results"], MAX_K))
        dist, ids = index.search_ids([like_id], k, allow=allow) if like_id is not None else index.search(vec[None, :], k, allow=allow)
        hits = [(d, i) for d, i in zip(dist[0], ids[0]) if i >= 0 and p["results"] > 0]
    if p["verbose"] > 0:
        print("search results:")
        print("distance path")
    for d, i in hits:
        print("  %f %s%s%s" % (d, image_paths[i], boxes.get(i, ""), " (+%d)" % more[i] if i in more else ""))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def compound_terms(p, image_paths, like_id, img_path, text):
    """The terms of a compound search as (source, value, kind): source "id" (an indexed image: value its id), "file" (an image file to load
    and encode) or "text"; kind "all" for the main query and every --and, "over" for every --not.  The main query is --like's indexed
    image, the positional image file or the positional text, as in a plain search; a --and / --not TERM with an image extension is an
    image, indexed when it equals a line of images.paths, and everything else is text."""
    terms = [("id", like_id, "all") if like_id is not None else ("file", img_path, "all") if img_path else ("text", text, "all")]
    for key, kind in (("and", "all"), ("not", "over")):
        for term in p.get(key, []):
            if is_image_file_extension(term):
                terms.append(("id", image_paths.index(term), kind) if term in image_paths else ("file", term, kind))
            else:
                terms.append(("text", term, kind))
    return terms


def _search_compound(clip_cpp_amd, clip, p, image_paths, like_id, img_path, text):
    """`search` with --and / --not: one Index.search_compound over the main query and the terms.  Every text term is encoded in one
    encode_texts call and every image file in one batch; an indexed image is its stored row."""
    terms = compound_terms(p, image_paths, like_id, img_path, text)
    texts = [value for source, value, _ in terms if source == "text"]
    files = [value for source, value, _ in terms if source == "file"]
    if files and clip.vision_config["n_layer"] <= 0:
        _err("main: the model at %s has no vision encoder: image queries need a vision or two-tower model" % p["model"])
        return 1
    if texts and clip.text_config["n_layer"] <= 0:
        _err("main: the model at %s has no text encoder: text queries need a two-tower model" % p["model"])
        return 1
    vecs = {}
    if texts:
        enc = np.asarray(clip.encode_texts([clip.tokenize(t) for t in texts], normalize=True), dtype=np.float32)
        vecs.update((("text", t), v) for t, v in zip(texts, enc))
    if files:
        L = clip_cpp_amd.lib()
        imgs = []
        try:
            for path in files:
                imgs.append(L.clip_image_u8_make())
                if not L.clip_image_load_from_file(os.fsencode(path), imgs[-1]):
                    _err("main: failed to load image from '%s'" % path)
                    return 1
            vecs.update((("file", f), v) for f, v in zip(files, _encode_batch(clip, L, imgs)))
        finally:
            for im in imgs:
                L.clip_image_u8_free(im)
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    for v in vecs.values():
        if index.dim != v.size:
            _err("main: the index holds %d-dimensional embeddings, the model makes %d" % (index.dim, v.size))
            return 1
    allow = None
    if p["in"]:
        allow = np.array([path.startswith(tuple(p["in"])) for path in image_paths], dtype=np.bool_)
    margin = p.get("not_margin", 0.0)
    query = [(value if source == "id" else vecs[(source, value)], kind) + ((margin,) if kind == "over" else ()) for source, value, kind in terms]
    k = max(1, min(p["results"], MAX_K))
    hits = []
    if len(index) > 0:                             # (the library refuses an empty index)
        dist, ids = index.search_compound([query], k, allow=allow, exclude_terms=True)
        hits = [(d, i) for d, i in zip(dist[0], ids[0]) if i >= 0 and p["results"] > 0]
    if p["verbose"] > 0:
        print("search results:")
        print("distance path")
    for d, i in hits:
        print("  %f %s" % (d, image_paths[i]))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def duplicate_groups(i, j, d):
    """Connected components of the graph whose edges are the pairs (i[t], j[t]) at distance d[t]: a list, in order of each group's lowest
    id, of [(id, distance to its nearest other member), ...] in id order.  Every id on an edge is in exactly one group of two or more."""
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    nearest = {}
    for a, b, dd in zip(np.asarray(i).tolist(), np.asarray(j).tolist(), np.asarray(d, dtype=np.float64).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)       # the root is the lowest id of the group
        for x in (a, b):
            if x not in nearest or dd < nearest[x]:
                nearest[x] = dd
    groups = {}
    for x in sorted(nearest):
        groups.setdefault(find(x), []).append((x, nearest[x]))
    return [groups[r] for r in sorted(groups)]


def component_groups(labels, nearest_distance):
    """The groups of Index.components' output in the structure of duplicate_groups: a list, in order of each group's lowest id, of
    [(id, distance to its nearest other member), ...] in id order, over the rows that have a near row (a finite nearest distance)."""
    labels = np.asarray(labels, dtype=np.int64)
    dist = np.asarray(nearest_distance, dtype=np.float32).astype(np.float64)
    ids = np.flatnonzero(np.isfinite(dist) & (labels >= 0))
    order = ids[np.argsort(labels[ids], kind="stable")]          # by group (its label is its lowest id), ids ascending within one
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    return [list(zip(g.tolist(), dist[g].tolist())) for g in np.split(order, cuts) if g.size]


def extent_groups(labels, centre, radius, diameter, reach, min_size=2, largest_first=False):
    """The groups of Index.extents' output over `labels`: a list of (centre id, radius, diameter, [(id, distance to its farthest member),
    ...] the other members in id order) over the groups of at least min_size members (the centre counts), in order of each group's lowest
    id, or, largest_first, largest first and equal sizes in order of the lowest id.  Rows with centre -1 are members of no group."""
    labels = np.asarray(labels, dtype=np.int64)
    centre = np.asarray(centre, dtype=np.int64)
    radius = np.asarray(radius, dtype=np.float32).astype(np.float64)
    diameter = np.asarray(diameter, dtype=np.float32).astype(np.float64)
    reach = np.asarray(reach, dtype=np.float32).astype(np.float64)
    ids = np.flatnonzero(centre >= 0)
    order = ids[np.argsort(labels[ids], kind="stable")]          # by group, ids ascending within one
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    found = [g for g in np.split(order, cuts) if g.size >= max(int(min_size), 1)]
    found.sort(key=lambda g: (-g.size if largest_first else 0, int(g[0])))
    out = []
    for g in found:
        c = int(centre[g[0]])
        rest = g[g != c]
        out.append((c, float(radius[c]), float(diameter[c]), list(zip(rest.tolist(), reach[rest].tolist()))))
    return out


def _print_extent_groups(found, image_paths):
    """`groups --extents` / `dedup --extents`: every group with its centre first; returns the largest diameter (0 without a group)"""
    for g, (c, radius, diameter, members) in enumerate(found):
        if g:
            print()
        print("  %f %f %s" % (radius, diameter, image_paths[c]))
        for i, d in members:
            print("  %f %s" % (d, image_paths[i]))
    return max([diameter for _, _, diameter, _ in found], default=0.0)


def album_groups(labels, parent_distance, min_size=2):
    """The albums of Index.modes' output: a list of (cover id, [(id, distance to its parent), ...] the other members in id order) over the
    albums of at least min_size rows (the cover counts), largest first, equal sizes in order of the cover's id.  Rows with label -1 are in
    no album."""
    labels = np.asarray(labels, dtype=np.int64)
    dist = np.asarray(parent_distance, dtype=np.float32).astype(np.float64)
    ids = np.flatnonzero(labels >= 0)
    order = ids[np.argsort(labels[ids], kind="stable")]          # by album (its label is its cover), ids ascending within one
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    albums = [(int(labels[g[0]]), g[g != labels[g[0]]]) for g in np.split(order, cuts) if g.size >= max(int(min_size), 1)]
    albums.sort(key=lambda a: (-a[1].size, a[0]))
    return [(cover, list(zip(g.tolist(), dist[g].tolist()))) for cover, g in albums]


def albums(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, albums=True)
    if p is None:
        _help(False, dict(verbose=1, db="."), albums=True)
        return 1
    if _refuse_gridded(p["db"], "albums"):
        return 1
    image_paths = _read_db(p)
    if image_paths is None:
        return 1
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the index's device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    labels, _, parent_distance, _ = index.modes(p["max_distance"], p["link"])
    groups = album_groups(labels, parent_distance, p["min_size"])
    if p["results"] is not None:
        groups = groups[:max(p["results"], 0)]
    if p["verbose"] > 0:
        print("albums:")
    for g, (cover, members) in enumerate(groups):
        if g:
            print()
        print(image_paths[cover])
        for i, d in members:
            print("  %f %s" % (d, image_paths[i]))
    print("main: %d albums, %d images" % (len(groups), sum(1 + len(m) for _, m in groups)))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def spread_lines(centres, reach, owner, paths):
    """The lines of `spread` for Index.spread's output: one per centre in pick order, "%f %s (+K)": the reach (inf for a seed or the first
    centre), the path and K, the number of other rows the centre owns."""
    centres = np.asarray(centres, dtype=np.int64)
    owner = np.asarray(owner, dtype=np.int64)
    owned = np.bincount(owner[owner >= 0], minlength=len(paths)) if owner.size else np.zeros(len(paths), dtype=np.int64)
    return ["%f %s (+%d)" % (float(r), paths[int(c)], int(owned[c]) - 1) for c, r in zip(centres.tolist(), np.asarray(reach, dtype=np.float32).tolist())]


def spread(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, spread=True)
    if p is None:
        _help(False, dict(verbose=1, db="."), spread=True)
        return 1
    if _refuse_gridded(p["db"], "spread"):
        return 1
    image_paths = _read_db(p)
    if image_paths is None:
        return 1
    seeds = []
    for path in p["from"]:
        if path not in image_paths:
            _err("main: '%s' is not in the database (paths are compared as written in %s)" % (path, PATHS_FILE))
            return 1
        seeds.append(image_paths.index(path))
    allow = None
    if p["in"]:
        allow = np.array([path.startswith(tuple(p["in"])) for path in image_paths], dtype=np.bool_)
        outside = [image_paths[i] for i in seeds if not allow[i]]
        if outside:
            _err("main: '%s' does not start with an --in prefix: a --from image must be one of the images picked from" % outside[0])
            return 1
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the index's device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    centres, reach, owner, _, cover = index.spread(p["results"], p["max_distance"], seeds or None, allow=allow)
    if p["verbose"] > 0:
        print("spread:")
    for line in spread_lines(centres, reach, owner, image_paths):
        print(line)
    print("main: %d images, every other image within %f of one of them" % (len(centres), cover))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def tree_groups(size, lo, hi, d, n_groups, eligible=None, min_size=2):
    """Exactly n_groups groups from the edges of Index.linkage (the whole tree, sorted): the tree without its n_groups - 1 longest edges.
    Returns (groups, longest edge kept, shortest edge dropped): groups in the structure of component_groups, [(id, distance to its
    nearest other member), ...] in id order (inf for a single image), only those of at least min_size images, largest first, equal sizes
    in order of the lowest id; the two distances are -inf / inf when no edge is kept / dropped.  Every `dedup -d R` with R from the first
    up to, but not including, the second finds these groups.  ValueError when the edges cannot give n_groups."""
    import clip_cpp_amd
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    d = np.asarray(d, dtype=np.float32)
    labels = clip_cpp_amd.cut_linkage(size, lo, hi, d, n_groups=n_groups, eligible=eligible)
    kept = int(np.count_nonzero(labels >= 0)) - int(n_groups)
    return (_label_groups(labels, lo[:kept], hi[:kept], d[:kept], min_size), float(d[kept - 1]) if kept > 0 else float("-inf"),
            float(d[kept]) if kept < d.size else float("inf"))


def _label_groups(labels, lo, hi, d, min_size):
    """The groups of a cut in the structure of component_groups: labels of the cut and the edges it kept -> [(id, distance of its
    shortest kept edge), ...] per group in id order (inf for a single row), only the groups of at least min_size rows, largest first,
    equal sizes in order of the lowest id"""
    nearest = np.full(labels.size, np.inf, dtype=np.float64)
    np.minimum.at(nearest, lo, d.astype(np.float64))
    np.minimum.at(nearest, hi, d.astype(np.float64))
    ids = np.flatnonzero(labels >= 0)
    order = ids[np.argsort(labels[ids], kind="stable")]
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    groups = [g for g in np.split(order, cuts) if g.size >= max(int(min_size), 1)]
    groups.sort(key=lambda g: (-g.size, int(g[0])))
    return [list(zip(g.tolist(), nearest[g].tolist())) for g in groups]


def sized_groups(size, lo, hi, w, n_groups, eligible=None, min_size=2):
    """`groups --core K`: exactly n_groups groups of at least min_size rows from the edges of Index.linkage_core (sorted), cut at the
    largest weight that gives them (clip_cpp_amd.cut_linkage_sized).  Returns (groups, radius, unfiled): groups in the structure and
    order of tree_groups, a member's distance being the smallest kept weight at it; unfiled: the eligible rows in no such group.
    ValueError when no weight gives n_groups."""
    import clip_cpp_amd
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    labels, radius = clip_cpp_amd.cut_linkage_sized(size, lo, hi, w, n_groups, min_size=min_size, eligible=eligible)
    kept = w <= np.float32(radius)
    groups = _label_groups(labels, lo[kept], hi[kept], w[kept], min_size)
    return groups, radius, int(np.count_nonzero(labels >= 0)) - sum(len(g) for g in groups)


def level_rows(size, d_sorted_lo, d_sorted_hi, d, rows=LEVEL_ROWS):
    """The table of `levels` from the edges of Index.linkage (sorted): up to `rows` positions evenly spaced over the merges, the last merge
    among them, each moved to the end of its run of equal distances, so that a row says what the cut at its distance gives: (distance,
    groups of two or more rows, rows in them, size of the largest group)."""
    lo, hi = np.asarray(d_sorted_lo, dtype=np.int64).tolist(), np.asarray(d_sorted_hi, dtype=np.int64).tolist()
    d = np.asarray(d, dtype=np.float32)
    e = d.size
    if e == 0:
        return []
    rows = max(1, min(int(rows), e))
    ends = sorted({int(np.searchsorted(d, d[(e * (r + 1)) // rows - 1], side="right")) for r in range(rows)})
    parent, size_of = list(range(size)), [1] * size
    groups = images = largest = 0
    out, done = [], 0
    for end in ends:
        for t in range(done, end):
            a, b = lo[t], hi[t]
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            while parent[b] != b:
                parent[b] = parent[parent[b]]
                b = parent[b]
            if a == b:
                continue
            if a > b:
                a, b = b, a
            groups += 1 - (size_of[a] > 1) - (size_of[b] > 1)
            images += (size_of[a] == 1) + (size_of[b] == 1)
            parent[b] = a
            size_of[a] += size_of[b]
            largest = max(largest, size_of[a])
        done = end
        out.append((float(d[end - 1]), groups, images, largest))
    return out


def _load_tree(p, command):
    """What `groups` and `levels` share: (paths, eligible or None, (lo, hi, d), extents) of the database's tree, or None after a message;
    extents: None, or with `groups --extents` (labels,) + Index.extents(labels) of the cut into -n groups"""
    import clip_cpp_amd
    if _refuse_gridded(p["db"], command):
        return None
    image_paths = _read_db(p)
    if image_paths is None:
        return None
    allow = None
    if p["in"]:
        allow = np.array([path.startswith(tuple(p["in"])) for path in image_paths], dtype=np.bool_)
    m = len(image_paths) if allow is None else int(allow.sum())
    if command == "groups" and p["results"] > m:
        _err("main: -n %d: there are only %d images to group" % (p["results"], m))
        return None
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the index's device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return None
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    core = p.get("core")
    edges = index.linkage(allow=allow) if core is None else index.linkage_core(core, allow=allow)[:3]
    extents, labels, refused = None, None, None
    if command == "groups" and core is not None:
        try:
            labels = clip_cpp_amd.cut_linkage_sized(len(image_paths), *edges, n_groups=p["results"], min_size=p["min_size"], eligible=allow)[0]
        except ValueError as e:
            refused = "main: -n %d: %s" % (p["results"], e)
    elif p.get("extents"):
        labels = clip_cpp_amd.cut_linkage(len(image_paths), *edges, n_groups=p["results"], eligible=allow)
    if p.get("extents") and labels is not None:
        extents = (labels,) + index.extents(labels, allow=allow)
    index.close()
    clip.close()
    if refused:
        print(refused)
        sys.stdout.flush()
        return None
    return image_paths, allow, edges, extents


def groups(argv):
    p = _parse(argv, build=False, groups=True)
    if p is None:
        _help(False, dict(verbose=1, db="."), groups=True)
        return 1
    loaded = _load_tree(p, "groups")
    if loaded is None:
        return 1
    image_paths, allow, (lo, hi, d), extents = loaded
    if p["core"] is None:
        found, kept, cut = tree_groups(len(image_paths), lo, hi, d, p["results"], allow, p["min_size"])
        closing = ("main: %d groups, %d of them with at least %d images, %d images in those; longest link kept %f, cut at %f"
                   % (p["results"], len(found), max(p["min_size"], 1), sum(len(g) for g in found), kept, cut))
    else:                                          # (_load_tree has made sure that the cut exists)
        found, radius, unfiled = sized_groups(len(image_paths), lo, hi, d, p["results"], allow, p["min_size"])
        closing = ("main: %d groups of at least %d images, %d images in those; cut at radius %f, %d images left unfiled"
                   % (len(found), max(p["min_size"], 1), sum(len(g) for g in found), radius, unfiled))
    if p["verbose"] > 0:
        print("groups:")
    if extents is not None:                        # the same groups in the same order, each with its centre first
        labels, centre, radius, diameter, reach, _ = extents
        closing += "; largest diameter %f" % _print_extent_groups(
            extent_groups(labels, centre, radius, diameter, reach, p["min_size"], largest_first=True), image_paths)
    else:
        for g, members in enumerate(found):
            if g:
                print()
            for i, dist in members:
                print("  %f %s" % (dist, image_paths[i]))
    print(closing)
    sys.stdout.flush()
    return 0


def levels(argv):
    p = _parse(argv, build=False, levels=True)
    if p is None:
        _help(False, dict(verbose=1, db="."), levels=True)
        return 1
    loaded = _load_tree(p, "levels")
    if loaded is None:
        return 1
    image_paths, allow, (lo, hi, d), _ = loaded
    table = level_rows(len(image_paths), lo, hi, d, p["results"])
    if p["verbose"] > 0:
        print("levels:")
        print("distance groups images largest")
    for dist, n_groups, images, largest in table:
        print("  %f %d %d %d" % (dist, n_groups, images, largest))
    print("main: %d images, %d levels" % (len(image_paths) if allow is None else int(allow.sum()), len(table)))
    sys.stdout.flush()
    return 0


def dedup(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, dedup=True)
    if p is None:
        _help(False, dict(verbose=1, db="."), dedup=True)
        return 1
    if _refuse_gridded(p["db"], "dedup"):
        return 1
    image_paths = _read_db(p)
    if image_paths is None:
        return 1
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the index's device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    prune = p.get("prune", False)                  # (the key exists only when --prune was given)
    labels, nearest, _ = index.components(p["max_distance"])
    groups = component_groups(labels, nearest)
    found, tail = None, ""
    if p.get("extents"):                           # the same groups in the same order, each with its centre first
        centre, radius, diameter, reach, _ = index.extents(labels)
        found = extent_groups(labels, centre, radius, diameter, reach, 2)
        tail = ", largest diameter %f" % max([g[2] for g in found], default=0.0)
    if p["verbose"] > 0 or not prune:
        if p["verbose"] > 0:
            print("duplicate groups:")
        if found is not None:
            _print_extent_groups(found, image_paths)
        else:
            for g, members in enumerate(groups):
                if g:
                    print()
                for i, d in members:
                    print("  %f %s" % (d, image_paths[i]))
    if prune:
        if found is not None:
            removed = sorted(i for _, _, _, members in found for i, _ in members)      # every member but the group's centre
        else:
            removed = [i for members in groups for i, _ in members[1:]]      # every member but the group's lowest id
        if removed:
            gone = set(removed)
            index.remove(removed)
            index.compact()
            _write_db(p, index, [path for i, path in enumerate(image_paths) if i not in gone])
        print("main: %d removed, %d kept%s" % (len(removed), len(image_paths) - len(removed), tail))
    else:
        print("main: %d groups, %d images%s" % (len(groups), sum(len(m) for m in groups), tail))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def neighbors(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, neighbors=True)
    if p is None:
        _help(False, dict(verbose=1, db=".", results=5), neighbors=True)
        return 1
    if _refuse_gridded(p["db"], "neighbors"):
        return 1
    image_paths = _read_db(p)
    if image_paths is None:
        return 1
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the index's device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    k = max(1, min(p["results"], MAX_K))
    dist, ids = index.knn_graph(k)
    if p["verbose"] > 0:
        print("neighbours:")
    for i, path in enumerate(image_paths):
        if i:
            print()
        print(path)
        for d, j in zip(dist[i], ids[i]):
            if j >= 0 and p["results"] > 0:
                print("  %f %s" % (d, image_paths[j]))
    print("main: %d images, %d neighbours each" % (len(image_paths), k if p["results"] > 0 else 0))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


VOTE_K = 10         # -k of `file` and `audit`: the voters counted per image
FILE_CLASSES = 3    # -n of `file`: the classes printed per image


def _parse_vote(argv, file):
    """The options of `file` (file=True: -t, -n and the images as well) and `audit`; None when they do not parse."""
    p = dict(threads=4, verbose=1, db=".", model="", k=VOTE_K, results=FILE_CLASSES, labels=None, rest=[])
    p["in"] = []
    takes = {"-m": "model", "--model": "model", "-v": "verbose", "--verbose": "verbose", "--db": "db", "-k": "k", "--labels": "labels", "--in": "in"}
    if file:
        takes.update({"-t": "threads", "--threads": "threads", "-n": "results", "--results": "results"})
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in takes:
            i += 1
            if i >= len(argv):
                return None
            key = takes[a]
            if key == "in":
                p["in"].append(argv[i])
            else:
                try:
                    p[key] = int(argv[i]) if key in ("threads", "verbose", "k", "results") else argv[i]
                except ValueError:
                    return None
        elif a in ("-h", "--help"):
            _help_vote(file, p)
            sys.exit(0)
        elif a.startswith("-"):
            print("main: unrecognized argument: %s" % a)
            return None
        elif not file:
            print("main: unexpected argument: %s" % a)
            return None
        else:
            p["rest"].append(a)
        i += 1
    if file and not p["rest"]:
        return None
    if not 1 <= p["k"] <= MAX_K:
        print("main: -k takes 1 ... %d, not %d" % (MAX_K, p["k"]))
        return None
    if p["results"] < 1:
        print("main: -n %d: file prints at least one class" % p["results"])
        return None
    return p


def _help_vote(file, p):
    if file:
        print("Usage: python -m clip_cpp_amd.image_search file [options] IMAGE [IMAGE ...]")
        print("\nFiles images by example: into which of your folders does each IMAGE go? The K nearest labelled images of an index built by")
        print("`build` vote with their folder (Index.vote); per IMAGE the N best folders are printed as `votes/voters distance folder ~ nearest")
        print("member`. An IMAGE that equals a line of %s is that indexed image: nothing is decoded, and it does not vote for itself." % PATHS_FILE)
    else:
        print("Usage: python -m clip_cpp_amd.image_search audit [options]")
        print("\nLists the images of an index built by `build` that lie in the wrong folder: every labelled image is filed by the vote of its K")
        print("nearest other labelled images (Index.vote_graph, one call; nothing is decoded or encoded), and those whose winning folder is not")
        print("their own are printed as `votes/voters distance path -> winning folder ~ nearest member of it`.")
    print("\nOptions:")
    print("  -h, --help: Show this message and exit")
    print("  -m <path>, --model <path>: overwrite path to model. Read from images.paths by default.")
    print("  -v <level>, --verbose <level>: Control the level of verbosity. 0 = minimum, 2 = maximum. Default: %d" % p["verbose"])
    if file:
        print("  -t N, --threads N: Number of threads to use for inference. Default: %d" % p["threads"])
        print("  -n N, --results N: classes printed per image. Default: %d" % p["results"])
    print("  --db <dir>: directory holding %s and %s. Default: %s" % (INDEX_FILE, PATHS_FILE, p["db"]))
    print("  -k K: voters counted per image (1 ... %d). Default: %d" % (MAX_K, p["k"]))
    print("  --labels FILE: lines `label<TAB>path` instead of the folders: the listed images carry that label, every other image is unlabelled")
    print("      (it may be asked about, it never votes). A path that is not in the database is an error.")
    print("  --in PREFIX: only images whose path starts with PREFIX vote%s. Repeatable." % ("" if file else " and are audited"))


def read_labels(image_paths, labels_file=None):
    """(labels int32 [n], names): the class of every indexed image and the classes' names, numbered in order of first appearance.  Without
    a file an image's class is the directory part of its line in images.paths, as written.  With one (lines `label<TAB>path`) the listed
    paths carry that label and every other image is unlabelled (-1); ValueError for a malformed line or a path that is not indexed."""
    names, number = [], {}
    labels = np.full(len(image_paths), -1, dtype=np.int32)

    def class_of(name):
        if name not in number:
            number[name] = len(names)
            names.append(name)
        return number[name]

    if labels_file is None:
        for i, path in enumerate(image_paths):
            labels[i] = class_of(os.path.dirname(path))
        return labels, names
    ids = {path: i for i, path in enumerate(image_paths)}
    with open(labels_file) as f:
        for n, line in enumerate(f.read().split("\n")):
            if not line:
                continue
            name, tab, path = line.partition("\t")
            if not tab:
                raise ValueError("%s line %d: expected `label<TAB>path`, not '%s'" % (labels_file, n + 1, line))
            if path not in ids:
                raise ValueError("%s line %d: '%s' is not in the database (paths are compared as written in %s)" % (labels_file, n + 1, path, PATHS_FILE))
            labels[ids[path]] = class_of(name)
    return labels, names


def _open_votes(p, command):
    """What `file` and `audit` share up to the index: (image paths, labels, class names, allowed set or None), or None with the message
    printed.  Nothing here loads a model."""
    if _refuse_gridded(p["db"], command):
        return None
    image_paths = _read_db(p)
    if image_paths is None:
        return None
    try:
        labels, names = read_labels(image_paths, p["labels"])
    except (OSError, ValueError) as e:
        _err("main: %s" % e)
        return None
    allow = None
    if p["in"]:
        allow = np.array([path.startswith(tuple(p["in"])) for path in image_paths], dtype=np.bool_)
    return image_paths, labels, names, allow


def vote_lines(classes, votes, dist, ids, counted, names, image_paths):
    """the lines of one image's vote: `  votes/voters distance class ~ nearest member` per class"""
    return ["  %d/%d %f %s ~ %s" % (v, counted, d, names[c], image_paths[j]) for c, v, d, j in zip(classes, votes, dist, ids) if c >= 0]


def file_images(argv):
    import clip_cpp_amd
    p = _parse_vote(argv, file=True)
    if p is None:
        _help_vote(True, dict(threads=4, verbose=1, db=".", k=VOTE_K, results=FILE_CLASSES))
        return 1
    opened = _open_votes(p, "file")
    if opened is None:
        return 1
    image_paths, labels, names, allow = opened
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    row_of = {path: i for i, path in enumerate(image_paths)}
    outside = [a for a in p["rest"] if a not in row_of]
    vecs = {}
    if outside:
        if clip.vision_config["n_layer"] <= 0:
            _err("main: the model at %s has no vision encoder: filing an image file needs a vision or two-tower model" % p["model"])
            return 1
        L = clip_cpp_amd.lib()
        for a in outside:
            im = L.clip_image_u8_make()
            try:
                if not L.clip_image_load_from_file(os.fsencode(a), im):
                    _err("main: failed to load image from '%s'" % a)
                    return 1
                vecs[a] = _encode_batch(clip, L, [im])[0]
            finally:
                L.clip_image_u8_free(im)
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    if vecs and index.dim != next(iter(vecs.values())).size:
        _err("main: the index holds %d-dimensional embeddings, the model makes %d" % (index.dim, next(iter(vecs.values())).size))
        return 1
    k, m = p["k"], min(p["results"], p["k"])
    voter = labels >= 0 if allow is None else (labels >= 0) & allow
    n_voters = int(voter.sum())
    stored = [row_of[a] for a in p["rest"] if a in row_of]
    res_stored = index.vote_ids(stored, k, labels, m=m, allow=allow) if stored else None
    res_out = index.vote(np.stack([vecs[a] for a in outside]), k, labels, m=m, allow=allow) if outside else None
    if p["verbose"] > 0:
        print("filing:")
    si = oi = 0
    for t, a in enumerate(p["rest"]):
        if t:
            print()
        print(a)
        if a in row_of:
            res, r, si = res_stored, si, si + 1
            counted = min(k, n_voters - int(voter[row_of[a]]))      # the image itself does not vote
        else:
            res, r, oi = res_out, oi, oi + 1
            counted = min(k, n_voters)
        for line in vote_lines(res[0][r], res[1][r], res[2][r], res[3][r], counted, names, image_paths):
            print(line)
    print("main: %d images, %d voters each" % (len(p["rest"]), k))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def audit(argv):
    import clip_cpp_amd
    p = _parse_vote(argv, file=False)
    if p is None:
        _help_vote(False, dict(verbose=1, db=".", k=VOTE_K))
        return 1
    opened = _open_votes(p, "audit")
    if opened is None:
        return 1
    image_paths, labels, names, allow = opened
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the index's device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    k = p["k"]
    classes, votes, dist, ids = index.vote_graph(k, labels, m=1, allow=allow)
    voter = labels >= 0 if allow is None else (labels >= 0) & allow
    n_voters = int(voter.sum())
    if p["verbose"] > 0:
        print("misfiled:")
    against = lonely = 0
    for i in np.flatnonzero(voter):                            # the audited images are the voters: labelled and, with --in, selected
        c = int(classes[i, 0])
        if c < 0:
            lonely += 1
        elif c != int(labels[i]):
            against += 1
            print("  %d/%d %f %s -> %s ~ %s" % (votes[i, 0], min(k, n_voters - 1), dist[i, 0], image_paths[i], names[c], image_paths[ids[i, 0]]))
    print("main: %d labelled images, %d filed against their neighbours, %d with no voter" % (n_voters, against, lonely))
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


DTYPE_NAMES = {0: "f32", 1: "f16", 3: "i8"}       # the dtype codes of a CLIPIDX1 header


def label(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, label=True)
    if p is None:
        _help(False, dict(threads=4, verbose=1, db=".", results=1), label=True)
        return 1
    if _refuse_gridded(p["db"], "label"):
        return 1
    image_paths = _read_db(p)
    if image_paths is None:
        return 1
    _, dim, dtype, _ = read_index_header(os.path.join(p["db"], INDEX_FILE))
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    if clip.text_config["n_layer"] <= 0:
        _err("main: the model at %s has no text encoder: text queries need a two-tower model" % p["model"])
        return 1
    if dim != clip.text_config["projection_dim"]:
        _err("main: the index holds %d-dimensional embeddings, the model makes %d" % (dim, clip.text_config["projection_dim"]))
        return 1
    names = p["rest"]
    labels = clip_cpp_amd.Index(clip, dim, dtype=DTYPE_NAMES[dtype])
    labels.add(clip.encode_texts([clip.tokenize(t) for t in names], normalize=True))      # as written: no prompt template
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    k = max(1, min(p["results"], len(names), MAX_K))
    dist, ids = labels.search_index(index, k)      # every image's stored row against the labels
    if p["verbose"] > 0:
        print("labels:")
    for i, path in enumerate(image_paths):
        if i:
            print()
        print(path)
        for d, j in zip(dist[i], ids[i]):
            if j >= 0 and p["results"] > 0:
                print("  %f %s" % (d, names[j]))
    print("main: %d images, %d labels each" % (len(image_paths), k if p["results"] > 0 else 0))
    sys.stdout.flush()
    index.close()
    labels.close()
    clip.close()
    return 0


def merge_refusal(target_model, target_hdr, source_dir, model_given):
    """Why the database in source_dir cannot be merged into a target with that model line and index header (version, dim, dtype, n), or
    None; read from the source's two files alone: no model and no device is needed."""
    model_line, paths = _read_paths(source_dir)
    hdr = read_index_header(os.path.join(source_dir, INDEX_FILE))
    if not model_line or hdr is None:
        return "no database in '%s' (%s or %s is missing or not a database file)" % (source_dir, PATHS_FILE, INDEX_FILE)
    if hdr[3] != len(paths):
        return "'%s': index files size missmatch" % source_dir
    if not model_given and model_line != target_model:
        return ("'%s' was built with the model %s, the target with %s: embeddings of two models cannot be compared (-m MODEL overrides "
                "this check when both paths name the same model)" % (source_dir, model_line, target_model))
    if hdr[1] != target_hdr[1]:
        return "'%s' holds %d-dimensional embeddings, the target %d-dimensional ones" % (source_dir, hdr[1], target_hdr[1])
    if hdr[2] != target_hdr[2]:
        return ("'%s' is stored as %s, the target as %s: build both with the same --dtype"
                % (source_dir, DTYPE_NAMES.get(hdr[2], hdr[2]), DTYPE_NAMES.get(target_hdr[2], target_hdr[2])))
    return None


def merge(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, merge=True)
    if p is None:
        _help(False, dict(verbose=1, db="."), merge=True)
        return 1
    if any(_refuse_gridded(db, "merge") for db in [p["db"]] + p["from"]):
        return 1
    model_given = bool(p["model"])
    paths = _read_db(p)
    if paths is None:
        return 1
    target_model = _read_paths(p["db"])[0]
    target_hdr = read_index_header(os.path.join(p["db"], INDEX_FILE))
    for source_dir in p["from"]:
        why = merge_refusal(target_model, target_hdr, source_dir, model_given)
        if why:
            _err("main: " + why)
            return 1
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])      # only the indexes' device: no image is encoded
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    target = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    known = set(paths)
    added = present = near = 0
    for source_dir in p["from"]:
        source_paths = _read_paths(source_dir)[1]
        source = clip_cpp_amd.Index.load(clip, os.path.join(source_dir, INDEX_FILE))
        nearest = None
        if p["max_distance"] is not None and len(target) and len(source):
            nearest = target.search_index(source, 1)      # before anything of this source is appended
        drop, keep = [], []
        for i, path in enumerate(source_paths):
            if path in known:
                present += 1
                drop.append(i)
            elif nearest is not None and nearest[1][i, 0] >= 0 and nearest[0][i, 0] <= np.float32(p["max_distance"]):
                near += 1
                drop.append(i)
                if p["verbose"] > 0:
                    print("  %f %s ~ %s" % (nearest[0][i, 0], path, paths[nearest[1][i, 0]]))
            else:
                known.add(path)
                keep.append(path)
        if drop:
            source.remove(drop)
            source.compact()
        if keep:
            target.append(source)
            paths.extend(keep)
            added += len(keep)
        source.close()
    if added:
        _write_db(p, target, paths)
    target.close()
    clip.close()
    print("main: %d added, %d already present, %d near duplicates skipped" % (added, present, near), flush=True)
    return 0


def _tile_suffix(rows, whole, r, arrow=""):
    """" [x,y,w,h]" of index row r when it is a tile, "" when it is the whole image"""
    return "" if whole[r] else "%s [%d,%d,%d,%d]" % ((arrow,) + tuple(rows[r, 1:]))


def match(argv):
    import clip_cpp_amd
    p = _parse(argv, build=False, match=True)
    if p is None:
        _help(False, dict(threads=4, verbose=1, db=".", results=5), match=True)
        return 1
    try:
        regions = read_regions(p["db"])
    except ValueError as e:
        _err("main: %s" % e)
        return 1
    if regions is None:
        _err("main: the database in '%s' was not built with --grid (it holds no %s): `match` compares images region by region; on a plain "
             "database use `search --like PATH` for one image or `neighbors` for all" % (p["db"], REGIONS_FILE))
        return 1
    image_paths = _read_db(p, regions)
    if image_paths is None:
        return 1
    grid, rows = regions
    groups = rows[:, 0]
    whole = np.ones(len(rows), dtype=np.bool_)
    whole[1:] = groups[1:] != groups[:-1]          # an image's first row is the whole image, the tiles follow
    query = p["rest"][0] if p["rest"] else None
    like_id = image_paths.index(query) if query in image_paths else None
    try:
        clip = clip_cpp_amd.Clip(p["model"], verbosity=p["verbose"])
    except RuntimeError:
        print("main: Unable to load model from %s" % p["model"])
        return 1
    k = max(1, min(p["results"], MAX_K))
    vecs = boxes = None
    if query is not None and like_id is None:      # an image file: its 1 + G * G regions are the query set
        if clip.vision_config["n_layer"] <= 0:
            _err("main: the model at %s has no vision encoder: image queries need a vision or two-tower model" % p["model"])
            return 1
        vecs, ok, _, boxes = clip.encode_image_files([query], normalize=True, n_threads=p["threads"], grid=grid)
        if not len(ok) or not ok[0]:
            _err("main: failed to load image from '%s'" % query)
            return 1
    index = clip_cpp_amd.Index.load(clip, os.path.join(p["db"], INDEX_FILE))
    if vecs is not None and index.dim != vecs.shape[1]:
        _err("main: the index holds %d-dimensional embeddings, the model makes %d" % (index.dim, vecs.shape[1]))
        return 1

    def show(dist, ids, qsuffix):
        for t, (d, r) in enumerate(zip(dist, ids)):
            if r >= 0 and p["results"] > 0:
                print("  %f %s%s%s" % (d, image_paths[groups[r]], _tile_suffix(rows, whole, r), qsuffix(t)))

    if query is None:                              # every image's nearest other images, by best region pair
        labels, dist, ids, qids = index.knn_graph_grouped(k, groups)
        if p["verbose"] > 0:
            print("matches:")
        for i, img in enumerate(labels):
            if i:
                print()
            print(image_paths[img])
            show(dist[i], ids[i], lambda t: _tile_suffix(rows, whole, qids[i, t], " <-"))
        print("main: %d images, %d matches each" % (len(labels), k if p["results"] > 0 else 0))
    else:
        if like_id is not None:
            own = np.flatnonzero(groups == like_id)
            dist, ids, qrows = index.search_ids_sets(own, [0, len(own)], k, groups=groups, exclude_own=True)
            qsuffix = lambda t: _tile_suffix(rows, whole, own[qrows[0, t]], " <-")
        else:
            dist, ids, qrows = index.search_sets(vecs, [0, len(vecs)], k, groups=groups)
            qsuffix = lambda t: "" if qrows[0, t] == 0 else " <- [%d,%d,%d,%d]" % tuple(boxes[qrows[0, t]])
        if p["verbose"] > 0:
            print("search results:")
            print("distance path")
        show(dist[0], ids[0], qsuffix)
    sys.stdout.flush()
    index.close()
    clip.close()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    commands = {"build": build, "update": update, "search": search, "dedup": dedup, "neighbors": neighbors, "label": label, "merge": merge, "match": match,
                "albums": albums, "spread": spread, "groups": groups, "levels": levels, "file": file_images, "audit": audit}
    if not argv or argv[0] not in commands:
        print("Usage: python -m clip_cpp_amd.image_search {build|search|dedup} [options] ...  (-h after the command for its options)")
        print("       python -m clip_cpp_amd.image_search update [options] dir [more dirs]  (an existing database brought in line with the disk)")
        print("       python -m clip_cpp_amd.image_search albums [options]  (the database grouped by content: albums, each with its most typical image as the cover)")
        print("       python -m clip_cpp_amd.image_search spread [options] -n N  (N images that between them cover the database: farthest-first selection)")
        print("       python -m clip_cpp_amd.image_search groups [options] -n N  (the database split into exactly N groups: the single-linkage tree, cut)")
        print("       python -m clip_cpp_amd.image_search levels [options]  (the table of distance against groups: which -d to give dedup)")
        print("       python -m clip_cpp_amd.image_search neighbors [options]  (every indexed image's nearest other images; search --like PATH for one)")
        print("       python -m clip_cpp_amd.image_search label [options] LABEL [LABEL ...]  (every indexed image's best-fitting labels)")
        print("       python -m clip_cpp_amd.image_search merge [options] --db DIR --from DIR2 [--from DIR3 ...]  (append databases, nothing encoded twice)")
        print("       python -m clip_cpp_amd.image_search match [options] [IMAGE]  (a --grid database: the images that share a region with IMAGE, or with each other)")
        print("       python -m clip_cpp_amd.image_search file [options] IMAGE [IMAGE ...]  (into which of your folders each IMAGE goes: its nearest labelled images vote)")
        print("       python -m clip_cpp_amd.image_search audit [options]  (the indexed images that lie in the wrong folder, by the vote of their neighbours)")
        return 1
    return commands[argv[0]](argv[1:])


if __name__ == "__main__":
    sys.exit(main())
