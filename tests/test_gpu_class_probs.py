"""GPU tier of the class probabilities of the exact index (clip_amd_index_class_probs[_ids | _device]; k_classes.hip).  all_probs and log_z
are compared with tests/class_probs_common.py, float64 over the complete distance list that range_search at radius 4 (or a search with
k = every row) returns, which has search's bits; classes / probs with the top m of the device's own all_probs, bit for bit.

Bounds (profiles/class_probs_accuracy.txt): the largest errors measured on an MI355X over the shape and layout cases below were
4.679e-6 relative for a probability and 3.815e-6 absolute for log_z; each bound is 4x its figure, the project's margin for v_exp_f32's
last place and the f32 accumulation order.  The relative figure is above softmax's 2.9e-7 because EVERY class is compared here, also
one of probability 1e-37: its term is exp2 of t = (d - m) scale near -120, and t, an f32, carries half a unit in its last place
(2^-18 there) plus the rounding of scale, which exp2 turns into a relative error of a few 1e-6 (softmax's test sees only the k nearest
rows, whose probabilities its finish computes in double).  So the probabilities of at least 1e-3, the ones a user reads, carry a bound
of their own: 5.426e-7 measured over the same cases, again 4x.  A probability below f32's smallest normal cannot carry a relative error: it
is compared absolutely against that value."""
import ctypes as C

import numpy as np
import pytest

from class_probs_common import class_probs_reference
from index_subset_common import DTYPES

pytestmark = pytest.mark.gpu

PROB_RTOL, LOGZ_ATOL = 4 * 4.679e-6, 4 * 3.815e-6
LIKELY, LIKELY_RTOL = 1e-3, 4 * 5.426e-7              # the probabilities a user reads: at least LIKELY, held to their own measured figure
TINY = float(np.finfo(np.float32).tiny)
POISON = -77.0
BASE = dict(dim=36, n=257, nq=17, n_classes=33, scale=100.0)
# one axis at a time around BASE; 513 classes: two windows, over 600 rows so that both hold rows
SHAPES = [BASE] + [dict(BASE, dim=d) for d in (4, 512)] + [dict(BASE, n=n) for n in (1, 63, 65)] + [dict(BASE, nq=q) for q in (1, 65)] + \
         [dict(BASE, n_classes=c) for c in (1, 2, 512)] + [dict(BASE, n_classes=513, n=600), dict(BASE, scale=1.0)] + \
         [dict(BASE, nq=65, n_classes=512), dict(BASE, nq=130)]    # two workgroups of 64 columns; four column tiles per wave, the last wave partial


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def raw(clip_lib, ix, q, labels, n_classes, m, scale, outs=None):
    """one clip_amd_index_class_probs call with n_classes as given: (ok, (classes, probs, log_z, all_probs))"""
    q, labels = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(labels, dtype=np.int32)
    o = outs or (np.empty((len(q), m), dtype=np.int32), np.empty((len(q), m), dtype=np.float32), np.empty(len(q), dtype=np.float32),
                 np.empty((len(q), n_classes), dtype=np.float32))
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ok = clip_lib.lib().clip_amd_index_class_probs(ix.handle, q.ctypes.data_as(f32p), len(q), labels.ctypes.data_as(i32p), n_classes, m, scale, None,
                                                   *[None if a is None else a.ctypes.data_as(i32p if a.dtype == np.int32 else f32p) for a in o])
    return ok, o


def check(got, full, labels, eligible, beta, n_classes):
    """got = (classes, probs, log_z, all_probs) of a call; full = (lims, dist, ids), the complete distance list of its queries"""
    classes, probs, log_z, allp = got
    want, want_z = class_probs_reference(*full, labels, eligible, beta, n_classes)
    big = want >= TINY
    rel = float(np.max(np.abs(allp[big] - want[big]) / want[big], initial=0.0))
    some = np.isfinite(want_z)
    err_z = float(np.max(np.abs(log_z[some] - want_z[some]), initial=0.0))
    likely = want >= LIKELY
    rel_likely = float(np.max(np.abs(allp[likely] - want[likely]) / want[likely], initial=0.0))
    assert rel <= PROB_RTOL and rel_likely <= LIKELY_RTOL and err_z <= LOGZ_ATOL
    assert np.all(np.abs(allp[~big] - want[~big]) <= TINY)
    assert np.all(np.isneginf(log_z[~some])) and np.all(allp[~some] == 0)
    # the m best classes of the device's own matrix by (probability descending, class ascending); a class of probability 0 is not reported
    m = classes.shape[1]
    order = np.lexsort((np.broadcast_to(np.arange(n_classes), allp.shape), -allp.astype(np.float64)), axis=1)[:, :m]
    top = np.take_along_axis(allp, order, axis=1)
    assert np.array_equal(classes, np.where(top > 0, order, -1)) and probs.tobytes() == top.tobytes()


def make_labels(rng, n, n_classes):
    labels = rng.integers(0, n_classes, n).astype(np.int32)
    labels[rng.random(n) < 0.1] = -1                                      # about a tenth unlabelled
    labels[0] = n_classes - 1                                             # (so that labels.max() + 1 is n_classes)
    return labels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join("%s%g" % kv for kv in s.items() if BASE[kv[0]] != kv[1]) or "base")
def test_shapes(clip, clip_lib, dtype, shape):
    dim, n, nq, n_classes, scale = (shape[key] for key in ("dim", "n", "nq", "n_classes", "scale"))
    rng = np.random.default_rng(dim + 7 * n + 11 * nq + 13 * n_classes)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rng.standard_normal((n, dim), dtype=np.float32))
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    labels = make_labels(rng, n, n_classes)
    full = ix.range_search(q, 4.0)
    for m in (1, min(5, n_classes)):                                      # 5 exceeds the classes that hold a row at n = 1
        check(ix.class_probs(q, labels, m=m, scale=scale, full=True), full, labels, np.ones(n, dtype=bool), scale, n_classes)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["one_class", "round_robin"])
def test_layout(clip, clip_lib, dtype, layout):
    n, dim, nq, n_classes = 600, 36, 17, 512                              # the two extremes of the bank and ordering scheme
    rng = np.random.default_rng(29)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rng.standard_normal((n, dim), dtype=np.float32))
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    labels = np.full(n, 7, dtype=np.int32) if layout == "one_class" else (np.arange(n) % n_classes).astype(np.int32)
    ok, got = raw(clip_lib, ix, q, labels, n_classes, 5, 100.0)
    assert ok
    check(got, ix.range_search(q, 4.0), labels, np.ones(n, dtype=bool), 100.0, n_classes)
    ok, again = raw(clip_lib, ix, q, labels, n_classes, 5, 100.0)
    assert ok and all(a.tobytes() == b.tobytes() for a, b in zip(got, again))      # two identical calls: identical bytes
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities(clip, clip_lib, dtype):
    n, dim, nq = 257, 36, 17
    rng = np.random.default_rng(31)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rng.standard_normal((n, dim), dtype=np.float32))
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    _, ids, sp, sz = ix.softmax(q, n, scale=100.0)
    want = np.zeros((nq, n), dtype=np.float32)
    np.put_along_axis(want, ids, sp, axis=1)
    # every row a class of its own: the matrix is softmax's probability of every row
    _, _, log_z, allp = ix.class_probs(q, np.arange(n), scale=100.0, full=True)
    big = want >= TINY
    assert np.all(np.abs(allp[big] - want[big]) <= PROB_RTOL * want[big]) and np.all(np.abs(allp[~big] - want[~big]) <= TINY)
    assert np.all(np.abs(log_z - sz) <= LOGZ_ATOL)
    # one class: its probability is exactly 1
    classes, probs, log_z, allp = ix.class_probs(q, np.zeros(n, dtype=np.int32), scale=100.0, full=True)
    assert np.all(classes == 0) and np.all(probs == 1.0) and np.all(allp == 1.0) and np.all(np.abs(log_z - sz) <= LOGZ_ATOL)
    # no labelled row
    classes, probs, log_z, allp = ix.class_probs(q, np.full(n, -1), scale=100.0, full=True)
    assert np.all(classes == -1) and np.all(probs == 0) and np.all(np.isneginf(log_z)) and allp.shape == (nq, 1) and np.all(allp == 0)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_eligibility(clip, clip_lib, dtype):
    n, dim, nq, n_classes = 257, 36, 17, 33
    rng = np.random.default_rng(37)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    labels = make_labels(rng, n, n_classes)
    ix = clip_lib.Index(clip, dim, dtype)
    ix.add(rows)
    allow = np.ones(n, dtype=bool)
    allow[32:96] = False                                                # two whole 32-row words
    allow[[5, 130, 256]] = False                                        # single rows
    ix.remove([7, 100, 255])
    el = ix.live_mask() & allow
    got = ix.class_probs(q, labels, m=5, scale=100.0, allow=allow, full=True)
    check(got, ix.range_search(q, 4.0, allow=allow), labels, el, 100.0, n_classes)
    # an index that only ever held the eligible rows: other chunks, so the same values to rounding
    y = clip_lib.Index(clip, dim, dtype)
    y.add(rows[el])
    _, _, yz, yp = y.class_probs(q, labels[el], scale=100.0, full=True)
    y.close()
    yp = np.pad(yp, ((0, 0), (0, n_classes - yp.shape[1])))
    assert np.all(np.abs(got[3] - yp) <= 2 * PROB_RTOL * yp + TINY) and np.all(np.abs(got[2] - yz) <= 2 * LOGZ_ATOL)
    # a stored row as the query, itself excluded = its vector as the query with its bit cleared, bit for bit
    for i in (3, 64, 128):
        one = allow.copy()
        one[i] = False
        a = ix.class_probs_ids([i], labels, m=5, scale=100.0, exclude_self=True, allow=allow, full=True)
        b = ix.class_probs(rows[i], labels, m=5, scale=100.0, allow=one, full=True)
        assert all(x.tobytes() == y_.tobytes() for x, y_ in zip(a, b))
    # the device form over poisoned buffers of one slot more: the bytes of the host form
    import torch
    words = torch.from_numpy(clip_lib.allow_words(allow, n).view(np.int64)).cuda()
    dq, dl = torch.from_numpy(q).cuda(), torch.from_numpy(labels).cuda()
    dc = torch.full((nq * 5 + 1,), int(POISON), dtype=torch.int32, device="cuda")
    dp, dz, da = (torch.full((s + 1,), POISON, dtype=torch.float32, device="cuda") for s in (nq * 5, nq, nq * n_classes))
    ix.class_probs_device(dq.data_ptr(), nq, dl.data_ptr(), n_classes, dc.data_ptr(), dp.data_ptr(), dz.data_ptr(), m=5, scale=100.0,
                          d_allow=words.data_ptr(), d_all_probs=da.data_ptr())
    clip.synchronize()
    for dev, h in zip((dc, dp, dz, da), got):
        assert dev[-1].item() == POISON and dev[:-1].cpu().numpy().tobytes() == np.ascontiguousarray(h).tobytes()
    # a device label outside 0 ... n_classes - 1 is an unlabelled row: it cannot set the minimum either (here it is each query's nearest)
    near = ix.search(q, 1, allow=allow)[1][:, 0]
    off = labels.copy()
    off[near] = -1
    dl[torch.from_numpy(near).cuda()] = n_classes + 5
    ix.class_probs_device(dq.data_ptr(), nq, dl.data_ptr(), n_classes, dc.data_ptr(), dp.data_ptr(), dz.data_ptr(), m=5, scale=100.0,
                          d_allow=words.data_ptr(), d_all_probs=da.data_ptr())
    clip.synchronize()
    host = ix.class_probs(q, off, m=5, scale=100.0, allow=allow, full=True)
    host = host[:3] + (np.pad(host[3], ((0, 0), (0, n_classes - host[3].shape[1]))),)      # (should the last class have lost its rows)
    for dev, h in zip((dc, dp, dz, da), host):
        assert dev[:-1].cpu().numpy().tobytes() == np.ascontiguousarray(h).tobytes()
    ix.close()


def test_refusals(clip, clip_lib, capfd):
    n, nq = 65, 2
    ix = clip_lib.Index(clip, 36, "f16")
    ix.add(np.random.default_rng(3).standard_normal((n, 36), dtype=np.float32))
    q = np.ones((nq, 36), dtype=np.float32)
    good = np.arange(n) % 4
    outs = (np.full((nq, 8), int(POISON), dtype=np.int32), np.full((nq, 8), POISON, dtype=np.float32), np.full(nq, POISON, dtype=np.float32),
            np.full((nq, 8), POISON, dtype=np.float32))
    for labels, n_classes, m, scale, o in ((np.where(good == 3, 4, good), 4, 1, 100.0, outs), (np.full(n, -2), 4, 1, 100.0, outs), (good, 4, 0, 100.0, outs),
                                            (good, 4, 5, 100.0, outs), (good, 0, 1, 100.0, outs), (good, 65537, 1, 100.0, outs),
                                            (good, 4, 1, float("nan"), outs), (good, 4, 1, 0.0, outs), (good, 4, 1, float("inf"), outs),
                                            (good, 4, 1, 100.0, (None,) + outs[1:]), (good, 4, 1, 100.0, outs[:1] + (None,) + outs[2:]),
                                            (good, 4, 1, 100.0, outs[:2] + (None, outs[3]))):
        ok, _ = raw(clip_lib, ix, q, labels, n_classes, m, scale, outs=o)
        assert ok is False and capfd.readouterr().err.strip()
        assert np.all(outs[0] == int(POISON)) and all(np.all(a == POISON) for a in outs[1:])
    ix.close()
