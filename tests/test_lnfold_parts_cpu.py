"""The reference's side of test_gpu_lnfold_parts.py, without a GPU: the numpy model of the LayerNorm fold's intermediate values
(lnfold_parts_common.py) is held to float64, the planted errors are shown to fall outside what the GPU tests accept, the exact cases are shown
to be exact, and the two hooks refuse on the host what the kernels do not take."""
import numpy as np
import pytest

import lnfold_parts_common as lp

F = np.float32


def _all_consumer_cases():
    seen = set()
    for tile in lp.CONSUMER_TILES:
        for tname in lp.TYPES:
            for sc in lp.consumer_plan(tile, tname):
                key = (tname, sc["M"], sc["N2"], sc["h"], sc["slotw"], sc["exact"], sc["epi"], tile == -1)
                if key not in seen:
                    seen.add(key)
                    yield tname, sc, tile == -1


def test_plans_cover_what_the_kernels_branch_on():
    cons = [(t, n, sc) for t in lp.CONSUMER_TILES for n in lp.TYPES for sc in lp.consumer_plan(t, n)]
    for tile in lp.CONSUMER_TILES:
        mine = [sc for t, n, sc in cons if t == tile]
        assert {sc["h"] for sc in mine} == set(lp.HS), tile                        # 1, 2, 5, 16, 17 (first masked chunk) and 32 units
        assert {sc["N2"] for sc in mine} == {128, 320} and {sc["epi"] for sc in mine} == {1, 2, 3}, tile
        assert {sc["exact"] for sc in mine} == {True, False}, tile
        assert len({sc["slotw"] == sc["h"] for sc in mine}) == 2, tile
        assert max(sc["M"] for sc in mine) == (77 if tile == -1 else 653 if tile == 320261 else 333), tile
        for sc in mine:
            units = sc["h"] // (64 if sc["slotw"] == 32 else sc["slotw"])
            assert tile == -1 or units <= 32
    for tile in lp.PRODUCER_TILES:
        assert {s for n in lp.TYPES for s in lp.producer_plan(tile, n)} >= ({(1, 64, 64), (77, 128, 192)} if tile == -1 else set()), tile
        assert len({s[1] for n in lp.TYPES for s in lp.producer_plan(tile, n)}) == 6, tile


@pytest.mark.parametrize("kind", ["plain", "common"])
def test_f32_statistics_stay_within_the_derived_bounds_of_float64(kind):
    """The emulation of the producers' statistics (every slot width) and of ln_row_final on them, against float64 of the same f32 rows, on the rows of
    the GPU tests (the hook's own x1 differs from this model's by f32 rounding only).  The bounds are those of lnfold_parts_common's docstring.
    Measured ratios error / bound, the largest over every slot and row: plain rows s 0.39, q 0.46, mean 0.06, rstd 0.15; common-mode rows
    (|mean| = 30 sigma, two channels at 100 x) s 0.51, q 0.54, mean 0.11, rstd 0.004."""
    worst = dict(s=0.0, q=0.0, mean=0.0, rstd=0.0)
    for tname, (M, h, K1) in [("f16", s) for s in lp.PRODUCER_SHAPES] + [("q4_0", (203, 320, 64)), ("q5_1", (333, 1088, 192))]:
        x1 = lp.producer_case(tname, M, h, K1, kind).x1_model
        mean64, var64 = lp.row64(x1)
        for slotw in (16, 32, 64):
            st = lp.producer_stats(x1, slotw)
            S, Q, bs, bq = lp.slot_bounds(x1, slotw)
            worst["s"] = max(worst["s"], (np.abs(st[:, :, 0] - S) / bs).max())
            worst["q"] = max(worst["q"], (np.abs(st[:, :, 1] - Q) / bq).max())
            if slotw == 16 and h > 512:
                continue                                  # more than 32 units: the tiled consumers do not take it
            m32, r32 = lp.ln_row_final(st, slotw, lp.EPS)
            mc, m2c = lp.chan64(st, slotw)                # the exact merge of the slots as stored ...
            worst["mean"] = max(worst["mean"], (np.abs(m32 - mc) / lp.mean_bound(st, slotw)).max())
            rc = 1.0 / np.sqrt(m2c / h + lp.EPS)
            worst["rstd"] = max(worst["rstd"], (np.abs(r32 / rc - 1) / lp.rstd_relerr(st, slotw, lp.EPS)).max())
            # ... which is the row's own (mean, variance) to within the slots' bounds
            assert np.all(np.abs(mc - mean64) <= bs.sum(0) / h * 1.01 + 1e-300)
            assert np.all(np.abs(m2c / h - var64) <= (bq.sum(0) + 2 * np.sqrt(bq.sum(0) * h * var64) + bs.sum(0) ** 2 / h) / h * 1.5 + 1e-300)
    print("ratios %s: %s" % (kind, worst))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_64_column_slots_are_the_pair_merge_of_32_column_slots():
    x1 = lp.producer_case("f16", 203, 320, 64, "common").x1_model
    assert np.array_equal(lp.producer_stats(x1, 64), lp.pairs_to_64(lp.producer_stats(x1, 32)))
    m_a, r_a = lp.ln_row_final(lp.producer_stats(x1, 64), 64, lp.EPS)
    m_b, r_b = lp.ln_row_final(lp.producer_stats(x1, 32), 32, lp.EPS)
    assert np.array_equal(m_a, m_b) and np.array_equal(r_a, r_b)


def test_exact_cases_are_exact():
    """eps = 0, h a power of two, equal slot sums, distinct slot q that sum to h 4^-j: ln_row_final's recurrence gives the same (mean, rstd) in float32
    and in float64 — mean_m and 2^j themselves —, and both FMAs of ln_apply are exact on the exact operands, so the GPU test may ask for bit equality."""
    n = 0
    for tname, sc, skinny in _all_consumer_cases():
        if not sc["exact"]:
            continue
        cs = lp.consumer_case(tname, sc["M"], sc["N2"], sc["h"], sc["slotw"], True)
        st = cs.st[:, :cs.M]
        q = st[:, :, 1]
        assert sc["slotw"] == sc["h"] or np.all(np.diff(q, axis=0) > 0), "distinct slot q"
        if not skinny:
            m32, r32 = lp.ln_row_final(st, cs.slotw, 0.0)
            m64, r64 = lp.ln_row_final(st, cs.slotw, 0.0, np.float64)
            assert m32.dtype == F and np.array_equal(m32.astype(np.float64), m64) and np.array_equal(r32.astype(np.float64), r64)
            assert np.array_equal(m64, cs.mean) and np.array_equal(r64, cs.rstd)
        mc, m2c = lp.chan64(st, cs.slotw)
        assert np.array_equal(mc, cs.mean) and np.array_equal(m2c / cs.h, cs.rstd ** -2.0)
        for with_mu in (True, False):
            qv = np.where(np.arange(cs.N2) < lp.QCOLS, lp.QSCALE, 1.0)
            mu = cs.mu.astype(np.float64) if with_mu else np.zeros(cs.M)
            rq = cs.rstd[:, None] * qv
            mq = (cs.mean - mu)[:, None] * rq
            inner = -cs.c.astype(np.float64) * mq + cs.bf.astype(np.float64) * qv
            v = cs.acc * rq + inner
            for a in (rq, mq, inner, v):
                assert np.array_equal(a.astype(F).astype(np.float64), a), "an f32 holds every intermediate value of ln_apply"
            assert np.array_equal(v, lp.consumer_value(cs.acc, cs.mean, cs.rstd, mu, cs.c.astype(np.float64), cs.bf.astype(np.float64), qv))
        n += 1
    assert n >= 20


def test_the_reference_alone_excepts_under_two_percent():
    """general cases, epilogue 1: the share of outputs whose float64 value lies within delta of a boundary between two fp16 values, where either
    neighbour passes: at most 2 % in every case, the GPU test's own condition, on the inputs that lnfold_parts_common.GENERAL_SEEDS fixes.  The
    largest over the cases of more than one row: 1.14 % (tiled kernels), 0.75 % (small-M kernel); a single row of 128 outputs excepts one at most."""
    worst = {False: 0.0, True: 0.0}
    for tname, sc, skinny in _all_consumer_cases():
        if sc["exact"] or sc["epi"] != 1:
            continue
        cs = lp.consumer_case(tname, sc["M"], sc["N2"], sc["h"], sc["slotw"], False)
        for with_mu in (True, False):
            v, lo, hi, exc = lp.consumer_expect(cs, 1, with_mu, skinny=skinny)
            assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi >= lo)
            worst[skinny] = max(worst[skinny], exc.mean() if cs.M > 1 else 0.0)          # (one row of 128 outputs: a share of 1 / 128 steps)
            assert exc.mean() <= 0.02, (tname, sc, with_mu, exc.mean())
    print("excepted shares: tiled %.4f small-M %.4f" % (worst[False], worst[True]))


MUTATIONS = {
    "slot index + 1": dict(slot_shift=1),
    "divisor h - 1": "divisor",
    "dropped cross term": dict(cross=False),
    "dropped last unit": dict(drop_last=True),
    "row index + 1": "row",
}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
def test_planted_errors_fall_outside_what_the_gpu_test_accepts(what):
    """ln_row_final with one planted off-by-one error: over the tiled consumer cases of the GPU test with more than one unit (and, for the row index, more
    than one row) the outputs leave the accepted window — in EVERY such case for the slot index, the divisor, the last unit and the row index; the cross
    term vanishes where the slot means are equal, so it shows in every GENERAL case.  Where the mean moves, so do mu_out's bits.

    One limit, stated plainly: a divisor of h - 1 moves rstd by 1 / (2 h) relative, and the GELU epilogues (2, 3) are held to
    gemm_exact_common.act_bound, whose own slack exceeds that once h > 320.  So the GELU cases at h = 1024, 1088 and 2048 CANNOT see this error and
    are left out of its count; it is the epilogue-1 cases, bit-exact or inside the fp16 window, that catch it, and they do at every h of the plan
    (each tile has epilogue-1 cases: test_plans_cover_what_the_kernels_branch_on)."""
    kw = MUTATIONS[what]
    hit = total = 0
    epi1_h = set()
    for tname, sc, skinny in _all_consumer_cases():
        units = sc["h"] // (64 if sc["slotw"] == 32 else sc["slotw"])
        if skinny or units < 2 or (what == "row index + 1" and sc["M"] < 2):
            continue
        if what == "divisor h - 1" and sc["epi"] != 1 and sc["h"] > 320:
            continue                          # 1 / (2 h) of rstd is below act_bound's own slack there; the epilogue-1 cases hold it at every h
        cs = lp.consumer_case(tname, sc["M"], sc["N2"], sc["h"], sc["slotw"], sc["exact"])
        st = cs.st[:, :cs.M]
        good_mean, _ = lp.ln_row_final(st, cs.slotw, cs.eps)
        if kw == "row":
            mean, rstd = lp.ln_row_final(st[:, np.minimum(np.arange(cs.M) + 1, cs.M - 1)], cs.slotw, cs.eps)
        elif kw == "divisor":
            mean, rstd = lp.ln_row_final(st, cs.slotw, cs.eps, divisor=cs.h - 1)
        else:
            mean, rstd = lp.ln_row_final(st, cs.slotw, cs.eps, **kw)
        v, lo, hi, _ = lp.consumer_expect(cs, sc["epi"], True)
        vm = lp.consumer_value(cs.acc, mean.astype(np.float64), rstd.astype(np.float64), cs.mu.astype(np.float64), cs.c.astype(np.float64),
                               cs.bf.astype(np.float64), np.where(np.arange(cs.N2) < (lp.QCOLS if sc["epi"] == 1 else 0), lp.QSCALE, 1.0))
        with np.errstate(over="ignore"):
            ym = (vm if sc["epi"] == 1 else lp.ACT[sc["epi"]](vm)).astype(np.float16).astype(F)
        outside = ((ym < lo) | (ym > hi)).mean()
        total += 1
        expect_hit = not (what == "dropped cross term" and cs.exact)
        if expect_hit:
            assert outside > 0.01, (what, tname, sc, outside)
            hit += 1
            if sc["epi"] == 1:
                epi1_h.add(sc["h"])
            if what in ("slot index + 1", "dropped last unit", "row index + 1") and not cs.exact:
                assert not np.array_equal(mean, good_mean), (what, tname, sc)
    assert hit >= 10, (what, hit, total)
    if what == "divisor h - 1":
        assert epi1_h >= {1024, 1088, 2048}, epi1_h


def test_hooks_refuse_on_the_host_what_the_kernels_do_not_take(clip_lib):
    """-3 before the device is looked for (no device would be -1), nothing written."""
    L = clip_lib.lib()
    for name in ("clip_amd_test_fold_producer", "clip_amd_test_fold_consumer"):
        assert name in clip_lib.AMD_SYMBOLS and hasattr(L, name)
    pc = lp.producer_case("q4_0", 8, 64, 64, "plain")

    def prod(what, **kw):
        a = dict(tid=pc.tid, raw=pc.raw, h=64, K1=64, A=pc.A, b1=pc.b1, resid=pc.resid, gamma=pc.gamma, xg_mu=pc.mu, tile1=64128, ldxg=None, M=None)
        a.update(kw)
        rc, x1, xg, stats, slotw = lp.call_producer(L, a["tid"], a["raw"], a["h"], a["K1"], a["A"], a["b1"], a["resid"], a["gamma"], a["xg_mu"],
                                                    a["tile1"], a["ldxg"], a["M"])
        assert rc == -3, (what, rc)
        assert np.all(np.isnan(x1)) and np.all(xg == 0xffff) and np.all(np.isnan(stats)) and slotw == -1, (what, "something was written")

    prod("h % 64", h=96)
    prod("h = 0", h=0)
    prod("M = 0", M=0)
    prod("K1 < 0", K1=-64)
    prod("M > 128 on the small-M kernel", tile1=-1, M=129)
    prod("tile -2", tile1=-2)
    prod("f32 weight", tid=0)
    prod("unknown type", tid=5)
    prod("ldxg < h", ldxg=56)
    prod("ldxg % 8", ldxg=68)
    for k in ("raw", "A", "b1", "resid", "gamma"):
        prod("no " + k, **{k: None, "M": 8})
    assert L.clip_amd_test_fold_producer(pc.tid, lp._vp(pc.raw), 64, 64, lp._fp(pc.A), 8, lp._fp(pc.b1), lp._fp(pc.resid), lp._fp(pc.gamma), None, 64128, 64,
                                         None, None, None, None) == -3

    cs = lp.consumer_case("q4_0", 8, 128, 128, 64, True)

    def cons(what, **kw):
        a = dict(tid=cs.tid, raw=cs.raw, N2=128, h=128, xg=cs.xg, st=cs.st, slotw=64, ln_mu=cs.mu, c=cs.c, bf=cs.bf, eps=0.0, epi2=1, qcols=0, qscale=1.0,
                 tile2=64128, M=None, slots=None)
        a.update(kw)
        rc, y, mu_out = lp.call_consumer(L, a["tid"], a["raw"], a["N2"], a["h"], a["xg"], a["st"], a["slotw"], a["ln_mu"], a["c"], a["bf"], a["eps"],
                                         a["epi2"], a["qcols"], a["qscale"], a["tile2"], a["M"], a["slots"])
        assert rc == -3, (what, rc)
        assert np.all(np.isnan(y)) and np.all(mu_out == 0), (what, "something was written")

    cons("slots * slotw != h", slots=3)
    cons("slots * slotw != h, slot width", slotw=32)
    cons("odd count of 32-column slots", h=96, slotw=32, slots=3)                   # (such an h is no multiple of 64 either)
    cons("more than 32 units on the tiled route", h=4096, slotw=64, slots=64)
    cons("more than 32 units, 16-column slots", h=1024, slotw=16, slots=64)
    cons("qcols % 4", qcols=6)
    cons("qcols > N2", qcols=132)
    cons("qcols < 0", qcols=-4)
    cons("M > 128 on the small-M kernel", tile2=-1, M=129)
    cons("epilogue 0", epi2=0)
    cons("epilogue 4", epi2=4)
    cons("tile -2", tile2=-2)
    cons("h % 64", h=96, slotw=96, slots=1)
    cons("N2 % 4", N2=126)
    cons("slotw = 0", slotw=0)
    cons("f32 weight", tid=0)
    for k in ("raw", "xg", "st", "c", "bf"):
        cons("no " + k, **{k: None, "M": 8, "slots": 2})
