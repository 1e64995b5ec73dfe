"""Shared by test_lnfold_parts_cpu.py and test_gpu_lnfold_parts.py: a numpy model of what passes between the two halves of the LayerNorm fold
(gemm_common.h resid_fold_tail / ln_pair32 / ln_row_final / ln_apply, k_skinny.hip), and the calls of the two hooks that cut the chain there
(include/clip_amd.h: clip_amd_test_fold_producer, clip_amd_test_fold_consumer).

The build runs -ffp-contract=off and the kernels reduce in a fixed order, so numpy float32 reproduces their statistics to the bit:

unit32_stats     the unit every tiled kernel reduces: 32 columns = 2 strips of 16; lane fgrp (0..3) holds columns 4 fgrp .. 4 fgrp + 3 of each strip and
                 sums its eight values as ((u0+u1)+(u2+u3)) + ((v0+v1)+(v2+v3)); the four lanes of a row go through the xor-16 / xor-32 butterfly
                 (sum4_fgrp: (l0+l1) + (l2+l3) in every lane, f32 addition commutes); mean = s / 32; the deviations about it are squared and summed in the same order.
pair32           ln_pair32: the Chan merge of two 32-column halves, shared by the 64-column producers and by the consumer of 32-column pairs.
producer_stats   the statistics buffer [h / slotw][M][2] a producer leaves: slotw 32 the units, 64 pair32 of two units with sum = mean64 * 64,
                 16 the small-M kernel's single strip (mean = s * (1/16)).
ln_row_final     the tiled consumers' merge: sequential over the units, k1 = 1/(t+1) and t/(t+1) f32 constants, k2 = w * (t/(t+1)), m2 = (m2 + q) + (d d) k2,
                 rstd = 1 / sqrt(m2 * (1 / (slots slotw)) + eps).  dtype = float64 evaluates the same recurrence in double (the exact cases compare the two).
chan64 / row64   float64: the Chan merge of given slots (also the model of the small-M consumer, which merges in another order with v_rcp), and the
                 plain (mean, variance) of a row.

Derived bounds (u = 2^-24; every figure follows the code, none is fitted to a kernel):

slot_bounds      |s - S| <= 5 u sum|x| for the five-level tree of 32 values (four levels for 16: the same 5 is kept).  The slot mean m_k = s / n is an exact
                 scaling, so E_m = |s - S| / n.  sum (x - m_k)^2 = Q + n (m - m_k)^2 exactly, and its f32 evaluation rounds each deviation (u, squared: 2 u),
                 each square (u) and five levels of sums of non-negative terms (5 u), 9 u relative with the subtraction counted once more:
                 |q - Q| <= 1.01 (9 u Q + n E_m^2).  A 64-column slot adds ln_pair32: d = m1 - m0 rounds (u |d| <= 2 u max|m|), mean64 = m0 + d / 2
                 rounds (u max|m|), s64 = 64 mean64 is exact: |s64 - S64| <= 64 ((E_m0 + E_m1) / 2 + 2 u max|m|); q64 = q0 + (q1 + 16 d d) sees d with the
                 error E_d = E_m0 + E_m1 + 2 u max|m| and rounds d d and two sums (3 u): |q64 - Q64| <= 1.01 (b_q0 + b_q1 + 16 (2 |d| E_d + E_d^2) + 3 u Q64).
mean_bound       E_mean of ln_row_final.  S = max |slot mean|; every running mean stays in [-S, S], |d| <= 2 S.  A step feeds in: the slot mean's own
                 rounding (s * invw with invw rounded: 2 u S) and the rounding of d (2 u S), both scaled by k1, the product d k1 with k1 rounded (4 u S k1) and
                 the addition (u S); the update mean' = (1 - k1) mean + k1 mu contracts earlier errors.  Sum over T units, sum k1 = H_T:
                 E_mean = 1.01 u S (T + 8 H_T).  Pairs add ln_pair32's 3 u S per unit, again scaled by k1: 11 H_T.
rstd_relerr      m2 is a sum of non-negative terms: 2 additions per unit -> (2 T + 4) u relative (the 4: d d, t/(t+1), w *, the product), and the cross terms
                 see d with the error E_d = E_mean + 4 u S: sum k2 (2 |d| E_d + E_d^2) <= 2 E_d sqrt(h) sqrt(m2) + h E_d^2 by Cauchy-Schwarz, i.e. relative
                 to m2 = h var: 2 E_d / sigma + (E_d / sigma)^2.  Then invh rounded, the product, the addition of eps: 3 u; the square root halves the
                 relative error; sqrtf and the division are allowed 2 u each (correctly rounded they take 1/2 u each):
                 rho = 1.01 (((2 T + 4) u + 2 E_d / sigma + (E_d / sigma)^2 + 3 u) / 2 + 4 u).
consumer_delta   ln_apply: rq = rstd q (u), mq = (mean - mu) rq (the subtraction u, the product u), v = fma(acc, rq, fma(-c, mq, b' q)) (b' q: u, each FMA: u of
                 its result): delta = 1.01 (|acc| rstd q (rho + u) + |c| rstd q (E_mean + |mean - mu| (rho + 3 u)) + u |b' q| + u |inner| + u |v|).
"""
import ctypes as C

import numpy as np

from oracle import ref

F = np.float32
U = 2.0 ** -24
POISON32 = 0x7fc00000
POISON16 = 0x7e00
MU_ROWS = 64                    # st_stride = M rounded up to this


def st_stride(M):
    return (M + MU_ROWS - 1) // MU_ROWS * MU_ROWS


# ---- the producers' statistics, float32, in the kernels' order ----
def _tree4(a):
    return (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])


def unit32_stats(x):
    """x f32 [..., 32] -> (s, q) f32 [...]"""
    v = np.ascontiguousarray(x, dtype=F).reshape(x.shape[:-1] + (2, 4, 4))       # strip, fgrp, column in the lane
    s = _tree4(_tree4(v[..., 0, :, :]) + _tree4(v[..., 1, :, :]))
    d = v - (s * F(1.0 / 32.0))[..., None, None, None]
    dd = d * d
    return s, _tree4(_tree4(dd[..., 0, :, :]) + _tree4(dd[..., 1, :, :]))


def strip16_stats(x, about_zero=False):
    v = np.ascontiguousarray(x, dtype=F).reshape(x.shape[:-1] + (4, 4))
    s = _tree4(_tree4(v))
    d = v if about_zero else v - (s * F(1.0 / 16.0))[..., None, None]
    return s, _tree4(_tree4(d * d))


def pair32(s0, q0, s1, q1, dtype=F):
    m0, m1 = s0 * dtype(1.0 / 32.0), s1 * dtype(1.0 / 32.0)
    d = m1 - m0
    return m0 + d * dtype(0.5), q0 + (q1 + (d * d) * dtype(16.0))


def producer_stats(x1, slotw):
    """-> f32 [h / slotw][M][2], what a producer with this slot width leaves for rows < M"""
    M, h = x1.shape
    if slotw == 16:
        s, q = strip16_stats(x1.reshape(M, h // 16, 16))
    else:
        s, q = unit32_stats(x1.reshape(M, h // 32, 32))
        if slotw == 64:
            mean, q = pair32(s[:, 0::2], q[:, 0::2], s[:, 1::2], q[:, 1::2])
            s = mean * F(64.0)
        else:
            assert slotw == 32
    return np.ascontiguousarray(np.stack([s.T, q.T], axis=-1), dtype=F)


def pairs_to_64(st32):
    """the 64-column statistics that the ln_pair32 of a 32-column producer's pairs gives"""
    mean, q = pair32(st32[0::2, :, 0], st32[0::2, :, 1], st32[1::2, :, 0], st32[1::2, :, 1])
    return np.stack([mean * F(64.0), q], axis=-1)


# ---- the consumers' merges ----
def ln_row_final(st, slotw, eps, dtype=F, divisor=None, cross=True, drop_last=False, slot_shift=0):
    """st [slots][rows][2] -> (mean, rstd) [rows] by ln_row_final's recurrence in `dtype`.  divisor / cross / drop_last / slot_shift plant the
    off-by-one errors of test_lnfold_parts_cpu.py; the defaults are the kernel."""
    st = np.asarray(st).astype(dtype)
    slots = st.shape[0]
    if slotw == 32:
        mu, q = pair32(st[0::2, :, 0], st[0::2, :, 1], st[1::2, :, 0], st[1::2, :, 1], dtype)
        w = dtype(64.0)
    else:
        w = dtype(slotw)
        mu, q = st[:, :, 0] * (dtype(1.0) / w), st[:, :, 1]
    units = mu.shape[0]
    mean, m2 = np.zeros(st.shape[1], dtype), np.zeros(st.shape[1], dtype)
    for t in range(units - (1 if drop_last else 0)):
        k1 = dtype(1.0) / dtype(t + 1)
        k2 = w * (dtype(t) / dtype(t + 1))
        j = min(t + slot_shift, units - 1)
        d = mu[j] - mean
        mean = mean + d * k1
        m2 = (m2 + q[j]) + ((d * d) * k2 if cross else dtype(0.0))
    invh = dtype(1.0) / (dtype(divisor) if divisor else dtype(slots) * dtype(slotw))
    with np.errstate(divide="ignore"):
        rstd = dtype(1.0) / np.sqrt(m2 * invh + dtype(eps))
    return mean, rstd


def chan64(st, slotw):
    """float64 Chan merge of the slots as given -> (mean, m2) [rows]"""
    st = np.asarray(st, dtype=np.float64)
    n, mean, m2 = 0.0, np.zeros(st.shape[1]), np.zeros(st.shape[1])
    for t in range(st.shape[0]):
        d = st[t, :, 0] / slotw - mean
        mean = mean + d * (slotw / (n + slotw))
        m2 = m2 + st[t, :, 1] + d * d * (n * slotw / (n + slotw))
        n += slotw
    return mean, m2


def row64(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(-1)
    return mean, ((x - mean[..., None]) ** 2).mean(-1)


# ---- derived bounds ----
def slot_bounds(x, slotw):
    """x [M][h] -> float64 (S, Q, bound_s, bound_q), each [slots][M]: the exact slot sums and squared deviations and the f32 emulation's distance from them"""
    M, h = x.shape
    v = np.asarray(x, dtype=np.float64).reshape(M, h // slotw, slotw)
    n = min(slotw, 32)
    vv = v.reshape(M, -1, n)
    S, A = vv.sum(-1), np.abs(vv).sum(-1)
    Q = ((vv - S[..., None] / n) ** 2).sum(-1)
    bs = 5 * U * A
    em = bs / n
    bq = 1.01 * (9 * U * Q + n * em * em) + 2.0 ** -140
    if slotw == 64:
        m0, m1 = S[:, 0::2] / 32, S[:, 1::2] / 32
        big = np.maximum(np.abs(m0), np.abs(m1))
        d = np.abs(m1 - m0)
        ed = em[:, 0::2] + em[:, 1::2] + 2 * U * big
        S, Q = v.sum(-1), ((v - v.mean(-1, keepdims=True)) ** 2).sum(-1)
        bq = 1.01 * (bq[:, 0::2] + bq[:, 1::2] + 16 * (2 * d * ed + ed * ed) + 3 * U * Q)
        bs = 64 * ((em[:, 0::2] + em[:, 1::2]) / 2 + 2 * U * big)
    return S.T, Q.T, bs.T, bq.T


def _slot_means(st, slotw):
    st = np.asarray(st, dtype=np.float64)
    return (st[0::2, :, 0] + st[1::2, :, 0]) / 64 if slotw == 32 else st[:, :, 0] / slotw, (np.abs(st[:, :, 0]) / slotw).max(0)


def mean_bound(st, slotw):
    """E_mean [rows] of ln_row_final on these statistics"""
    mu, S = _slot_means(st, slotw)
    T = mu.shape[0]
    H = sum(1.0 / (t + 1) for t in range(T))
    return 1.01 * U * S * (T + (11 if slotw == 32 else 8) * H) + 2.0 ** -140


def rstd_relerr(st, slotw, eps, skinny=False):
    """rho of the module docstring; skinny: the small-M consumer — every slot's way to the root is at most ceil(slots / 16) + 4 merges of two additions
    each (16 threads per row; with 32 it is ceil(slots / 32) + 5, no more where slots > 16, and below that the extra level adds an empty lane's
    zeros exactly: skinny_mean_bound), v_rcp_f32 taken at the same assumed 1 ulp as there, the cross term d d (n0 n1 inv) takes 6 u (d d, n0 n1, the reciprocal's 2 u, two products), m2 / n and + eps 2 u, E_mean as skinny_mean_bound."""
    mu, S = _slot_means(st, slotw)
    T = (st.shape[0] + 15) // 16 + 4 if skinny else mu.shape[0]
    _, m2 = chan64(st, slotw)
    sigma = np.sqrt(m2 / (st.shape[0] * slotw) + eps)
    ed = ((skinny_mean_bound(st, slotw) if skinny else mean_bound(st, slotw)) + 4 * U * S) / sigma
    return 1.01 * (((2 * T + (6 if skinny else 4)) * U + 2 * ed + ed * ed + (2 if skinny else 3) * U) / 2 + 4 * U)


def consumer_value(acc, mean, rstd, mu, c, bf, qv):
    """float64 q (rstd (acc - (mean - mu) c) + b'), [M][N]"""
    return qv * (rstd[:, None] * (acc - (mean - mu)[:, None] * c) + bf)


def consumer_delta(acc, mean, rstd, mu, c, bf, qv, e_mean, rho):
    dm = np.abs(mean - mu)[:, None]
    rq = rstd[:, None] * qv
    inner = -c * ((mean - mu)[:, None] * rq) + bf * qv
    v = acc * rq + inner
    return 1.01 * (np.abs(acc) * rq * (rho[:, None] + U) + np.abs(c) * rq * (e_mean[:, None] + dm * (rho[:, None] + 3 * U)) + U * np.abs(bf * qv) +
                   U * np.abs(inner) + U * np.abs(v)) + 2.0 ** -140


def f16_window(v, delta):
    """(lo, hi) f32: the fp16 roundings of v - delta and v + delta.  An fp16 output is accepted iff lo <= y <= hi: that is fp16(v) itself, or either
    neighbour where a boundary between two fp16 values lies within delta of v.  lo != hi marks the excepted outputs."""
    with np.errstate(over="ignore"):
        return (v - delta).astype(np.float16).astype(F), (v + delta).astype(np.float16).astype(F)


# ---- inputs ----
def exact_stats(M, h, slotw):
    """-> (st f32 [slots][st_stride][2], mean [M], rstd [M]).  Row m: every slot mean is mean_m = ((5 m) % 17 - 8) / 8, the slot q values are distinct
    and sum to h 4^-j, j = m % 4, so with eps = 0 the variance is 4^-j and rstd = 2^j.  The rows past M hold NaN: no kernel may use them."""
    slots = h // slotw
    assert slots & (slots - 1) == 0 and h & (h - 1) == 0
    m = np.arange(M)
    mean = ((5 * m) % 17 - 8) / 8.0
    j = m % 4
    t = np.arange(slots)[:, None]
    q = 4.0 ** -j[None, :] * slotw * (slots + 1 + 2 * t) / (2.0 * slots)
    assert np.allclose(q.sum(0), h * 4.0 ** -j, rtol=0, atol=0)
    st = np.full((slots, st_stride(M), 2), np.nan, dtype=F)
    st[:, :M, 0] = (mean * slotw)[None, :]
    st[:, :M, 1] = q
    assert np.array_equal(st[:, :M, 1].astype(np.float64), q)
    return st, mean, 2.0 ** j


def general_stats(rng, M, h, slotw, spread=0.05):
    """Unequal slot means (spread sigma about a per-row level of up to 0.12 sigma), per-row variance scale 4^-(m % 3): every row has its own (mean, rstd).
    The levels are kept small against sigma because E_mean grows with max |slot mean|: at 32 units the window of consumer_expect then excepts ~1 % of the
    outputs (test_lnfold_parts_cpu.py holds the share under 2 %); the cross term still moves rstd by spread^2 / 2 = 1.25e-3, 2.5 fp16 half-ulps.
    NaN in the rows past M."""
    slots = h // slotw
    m = np.arange(M)
    var = 4.0 ** -(m % 3) * (1 + 0.5 * rng.random(M))
    level = 0.02 * ((7 * m) % 13 - 6) * np.sqrt(var)
    mu = level[None, :] + spread * np.sqrt(var)[None, :] * rng.standard_normal((slots, M))
    st = np.full((slots, st_stride(M), 2), np.nan, dtype=F)
    st[:, :M, 0] = mu * slotw
    st[:, :M, 1] = slotw * var[None, :] * (0.5 + rng.random((slots, M)))
    return st


def row_offsets(M):
    """ln_mu: multiples of 1/4, another one for every row"""
    return (((3 * np.arange(M)) % 9 - 4) / 4.0).astype(F)


def common_mode_rows(rng, M, h):
    """residual rows with |mean| = 30 sigma and two outlier channels at 100 x"""
    r = rng.standard_normal((M, h))
    r[:, rng.choice(h, size=2, replace=False)] *= 100.0
    sigma = r.std(1, keepdims=True)
    sign = np.where(np.arange(M) % 2, -1.0, 1.0)[:, None]
    return (r + 30.0 * sigma * sign).astype(F)


# ---- the hooks ----
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def call_producer(L, tid, raw, h, K1, A, b1, resid, gamma, xg_mu, tile1, ldxg=None, M=None):
    """-> rc, x1 [M][h], xg u16 [M][ldxg], stats f32 [slots][st_stride][2] (None unless rc in (0, -6)), slotw.  Outputs the hook did not write hold 0xff bytes."""
    M = A.shape[0] if M is None else M
    ldxg = h if ldxg is None else ldxg
    x1 = np.full((max(M, 1), max(h, 1)), np.nan, dtype=F)
    xg = np.full((max(M, 1), max(ldxg, 1)), 0xffff, dtype=np.uint16)
    stats = np.full(max(h // 16, 1) * st_stride(max(M, 1)) * 2, np.nan, dtype=F)
    slotw = C.c_int(-1)
    rc = L.clip_amd_test_fold_producer(tid, _vp(raw), h, K1, _fp(A), M, _fp(b1), _fp(resid), _fp(gamma), _fp(xg_mu), tile1, ldxg, _fp(x1), _vp(xg),
                                       _fp(stats), C.byref(slotw))
    st = None
    if rc in (0, -6):
        slots = h // slotw.value
        st = stats[:slots * st_stride(M) * 2].reshape(slots, st_stride(M), 2)
    return rc, x1, xg, st if st is not None else stats, slotw.value


def call_consumer(L, tid, raw, N2, h, xg16, st, slotw, ln_mu, c, bf, eps, epi2, qcols, qscale, tile2, M=None, slots=None):
    """-> rc, y f32 [M][N2], mu_out f32 [st_stride]; xg16: float16 [M][h]"""
    M = xg16.shape[0] if M is None else M
    slots = st.shape[0] if slots is None else slots
    y = np.full((max(M, 1), max(N2, 1)), np.nan, dtype=F)
    mu_out = np.zeros(st_stride(max(M, 1)), dtype=F)
    rc = L.clip_amd_test_fold_consumer(tid, _vp(raw), N2, h, _vp(xg16), M, _fp(st), slots, slotw, _fp(ln_mu), _fp(c), _fp(bf), eps, epi2, qcols, qscale,
                                       tile2, _fp(y), _fp(mu_out))
    return rc, y, mu_out


def type_id(tname):
    return ref.GGML_TYPES[tname]


# ---- cases, built once and shared (the tests leave them unchanged) ----
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


QCOLS, QSCALE, EPS = 100, 0.125, float(F(1e-5))
_cases = {}


def _gelu_tanh(x):
    return 0.5 * x * (1 + np.tanh(0.7978845608028654 * x * (1 + 0.044715 * x * x)))


def _gelu_quick(x):
    with np.errstate(over="ignore"):
        return x / (1 + np.exp(-1.702 * x))


ACT = {2: _gelu_tanh, 3: _gelu_quick}

# The general cases' seeds, (type, M, N2, h, slot width) -> seed, 1 where not listed.  One row of 128 outputs excepts in steps of 1 / 128, so the
# single-row cases below take another seed to stay under the share; constants, so that a later change to a bound cannot change the inputs.
GENERAL_SEEDS = {("f16", 1, 128, 1088, 64): 3, ("f16", 1, 128, 2048, 2048): 2, ("q4_0", 1, 128, 320, 16): 2, ("q4_0", 1, 128, 320, 64): 2,
                 ("q5_1", 1, 128, 320, 64): 2, ("q5_1", 1, 128, 1088, 16): 3}


def consumer_case(tname, M, N2, h, slotw, exact, seed=0):
    """Operands known exactly (gemm_exact_common.exact_case: weights, c, b' multiples of 2^-6, the operand integer-valued, every partial sum an exact
    f32) with planted statistics: exact_stats (eps = 0) or general_stats (eps = 1e-5).  mean / rstd: float64, the exact merge of the planted slots."""
    import gemm_exact_common as ge
    key = (tname, M, N2, h, slotw, exact, seed)
    if key in _cases:
        return _cases[key]
    if not exact and seed == 0:
        # the share of excepted outputs is a condition of the GPU test (2 % per case), so the inputs are chosen for it: GENERAL_SEEDS, fixed here;
        # test_lnfold_parts_cpu.py asserts the share for the reference alone (the float64 values and the derived delta, no kernel)
        _cases[key] = consumer_case(tname, M, N2, h, slotw, False, GENERAL_SEEDS.get((tname, M, N2, h, slotw), 1))
        return _cases[key]
    rng = np.random.default_rng([seed, M, N2, h, slotw, int(exact), ge.WTYPES.index(tname)])
    xmax = min(4, ge.xmax_for(tname, h))
    ec = ge.exact_case(rng, tname, 1, N2, h, xmax)                 # the weight; its one-row product is not used
    X = rng.integers(-xmax, xmax + 1, size=(M, h)).astype(np.float64)
    acc = X @ ec.W.T                                               # exact: multiples of 2^-6 below 2^17, float64 holds every partial sum
    assert np.array_equal(acc * ge.UNIT, np.rint(acc * ge.UNIT)) and np.abs(acc).max() * ge.UNIT <= ge.BUDGET
    c = (rng.integers(-4 * ge.UNIT, 4 * ge.UNIT + 1, size=N2) / ge.UNIT).astype(F)
    if exact:
        st, mean, rstd = exact_stats(M, h, slotw)
        eps = 0.0
    else:
        st = general_stats(rng, M, h, slotw)
        eps = EPS
        mean, m2 = chan64(st[:, :M], slotw)
        rstd = 1.0 / np.sqrt(m2 / h + eps)
    _cases[key] = Case(tname=tname, tid=type_id(tname), M=M, N2=N2, h=h, slotw=slotw, exact=exact, raw=ec.raw, xg=X.astype(np.float16), acc=acc, c=c,
                       bf=ec.bias, st=st, eps=eps, mean=mean, rstd=rstd, mu=row_offsets(M))
    return _cases[key]


def consumer_expect(cs, epi2, with_mu, mean=None, rstd=None, skinny=False):
    """-> (v, lo, hi, excepted): v the float64 pre-activation value; an fp16 output y (widened) passes iff lo <= y <= hi.  Epilogue 1: the fp16 window of
    v +- delta (delta = 0 for the exact cases: bit equality; skinny: the small-M consumer's E_mean and rho); 2 / 3: act(v) +- (act_bound + 1.13 delta), the activations being 1.13-Lipschitz."""
    import gemm_exact_common as ge
    qv = np.where(np.arange(cs.N2) < (QCOLS if epi2 == 1 else 0), QSCALE, 1.0)
    mu = cs.mu.astype(np.float64) if with_mu else np.zeros(cs.M)
    mean = cs.mean if mean is None else mean
    rstd = cs.rstd if rstd is None else rstd
    c, bf = cs.c.astype(np.float64), cs.bf.astype(np.float64)
    v = consumer_value(cs.acc, mean, rstd, mu, c, bf, qv)
    if cs.exact:
        delta = np.zeros_like(v)
    else:
        st = cs.st[:, :cs.M]
        e_mean = skinny_mean_bound(st, cs.slotw) if skinny else mean_bound(st, cs.slotw)
        delta = consumer_delta(cs.acc, cs.mean, cs.rstd, mu, c, bf, qv, e_mean, rstd_relerr(st, cs.slotw, cs.eps, skinny))
    if epi2 == 1:
        lo, hi = f16_window(v, delta)
    else:
        g = ACT[epi2](v)
        b = ge.act_bound(g, v) + 1.13 * delta
        lo, hi = (g - b).astype(F), (g + b).astype(F)
    return v, lo, hi, lo != hi


def producer_case(tname, M, h, K1, kind, seed=0):
    """kind 'plain': the rows of test_gpu_kernels._lnfold_case (outlier channels, a small common mode); 'common': |mean| = 30 sigma, two channels at 100 x"""
    key = ("p", tname, M, h, K1, kind, seed)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng([seed, M, h, K1, kind == "common"])
    tid = type_id(tname)
    W = (rng.standard_normal((h, K1)) * 0.02).astype(F)
    W[:, rng.integers(0, K1, size=max(1, K1 // 128))] *= 8.0
    raw = ref.quantize(tid, W)
    A = rng.standard_normal((M, K1)).astype(F)
    if kind == "common":
        resid = common_mode_rows(rng, M, h)
    else:
        r = rng.standard_normal((M, h)) * 2.5
        r[:, rng.integers(0, h, size=2)] *= 20.0
        resid = (r + 0.3).astype(F)
    b1 = (rng.standard_normal(h) * 0.1).astype(F)
    gamma = (1 + rng.standard_normal(h) * 0.2).astype(F)
    mu = resid.astype(np.float64).mean(1).astype(F)                # the centred form's offsets: the means of the incoming rows
    Wd = ref.dequantize(tid, raw, h, K1).astype(np.float64)
    x1_model = (resid + (A.astype(np.float16).astype(np.float64) @ Wd.T + b1)).astype(F)      # the rows a kernel leaves, to within its f32 rounding
    _cases[key] = Case(tname=tname, tid=tid, M=M, h=h, K1=K1, raw=raw, A=A, resid=resid, b1=b1, gamma=gamma, mu=mu, x1_model=x1_model)
    return _cases[key]


def expected_xg(x1, mu, gamma):
    """((x1 - mu) * gamma).astype(float16) in float32 -> the raw bits"""
    m = np.zeros(x1.shape[0], F) if mu is None else mu
    with np.errstate(over="ignore"):
        return ((x1 - m[:, None]) * gamma[None, :]).astype(np.float16).view(np.uint16)


def skinny_mean_bound(st, slotw):
    """The small-M consumer (k_skinny.hip): TPR = 16 or 32 threads per row, by the instantiation; thread `sub` merges slots sub, sub + TPR, ...
    sequentially (ceil(slots / TPR) merges at most), then log2(TPR) butterfly levels, the lower lanes' aggregate first: ceil(slots / 16) + 4 merges on a
    slot's way to the root with 16 threads, ceil(slots / 32) + 5 with 32.  The first count is the larger one whenever slots > 16.  With slots <= 16 and
    32 threads the lanes that hold slots are a prefix of the row's lanes, so the fifth level merges lane 0's aggregate with an empty one (n1 = 0):
    mean = m0 + d * 0 exactly, and 1 + 4 stands there too.  A merge is mean = m0 + d (n1 inv), inv = v_rcp(n): d rounds (2 u S), n1 inv carries the
    reciprocal's error and its own u, the product u, the addition u S; a merge is a convex combination, so the errors of its two inputs do not add
    but the larger one passes on.  The slot mean s * invw: 2 u S.

    v_rcp_f32's accuracy is an ASSUMPTION here: 1 ulp = 2 u relative, the figure of a comment in gemm_common.h; neither this project's documents
    nor an ISA text that could be consulted states it.  With it a merge costs 4 u of |d| <= 2 S, 8 u S, and 11 u S in all:
    E = 1.01 u S (2 + 11 (ceil(slots / 16) + 4)).  Because of the assumption the GPU tests do not rest the small-M kernel's mean on this figure
    alone: they also hold its measured error to 4 x the tiled kernels' on the same rows (mean_ratio_pair)."""
    S = (np.abs(np.asarray(st, dtype=np.float64)[:, :, 0]) / slotw).max(0)
    return 1.01 * U * S * (2 + 11 * ((st.shape[0] + 15) // 16 + 4)) + 2.0 ** -140


def mean_ratio_pair(mu_small, st, slotw, mean64, extra=0.0):
    """The small-M consumer's mean next to the tiled kernels' on the same rows, each as error against float64 / (mean_bound + extra), [rows] each.
    The tiled kernels' mean is ln_row_final in f32 on the statistics `st` (the GPU tests hold every tiled kernel's mu_out to it bit for bit), so
    it needs no launch.  v_rcp_f32's accuracy not being documented, the GPU tests assert max(small) <= 4 max(tiled)."""
    den = mean_bound(st, slotw) + extra
    tiled = ln_row_final(st, slotw, EPS)[0].astype(np.float64)
    return np.abs(np.asarray(mu_small, dtype=np.float64) - mean64) / den, np.abs(tiled - mean64) / den


# ---- what test_gpu_lnfold_parts.py runs (test_lnfold_parts_cpu.py checks the reference's side of the same cases) ----
TYPES = ["f16", "q4_0", "q5_1"]
PRODUCER_TILES = [64064, 128064, 64128, 128128, 160128, 192128, 65064, 65128, 160256, 256256, 256259, 3065128, 0, -1]
CONSUMER_TILES = PRODUCER_TILES + [256261, 320261, 256260]
HS = [64, 128, 320, 1024, 1088, 2048]                 # 1, 2, 5, 16, 17 and 32 merge units of 64 columns
PRODUCER_SHAPES = [(1, 64, 64), (77, 128, 192), (203, 320, 64), (333, 1088, 192), (203, 1024, 64), (77, 2048, 192)]


def producer_plan(tile, tname):
    """three (M, h, K1) of PRODUCER_SHAPES per (tile, type), rotating: a tile sees all six over the three types.  The small-M kernel takes M <= 128
    (128 itself once); the split-K code gets K1 = 384, six K-tiles, so that it does split."""
    i = PRODUCER_TILES.index(tile) + 3 * TYPES.index(tname)
    out = []
    for k in range(3):
        M, h, K1 = PRODUCER_SHAPES[(i + k) % 6]
        if tile == -1 and M > 128:
            M = 128 if M == 333 else 77
        if tile // 1000000 > 1:
            K1 = 384
        out.append((M, h, K1))
    return out


_CONSUMER_SPECS = [   # (h, slot width: 64 / 32 (pairs) / 'h' (the entry kernels' single slot), exact statistics), four per weight type
    (64, 64, True), (1088, 32, False), (1024, 64, False), (2048, "h", False),
    (128, 32, True), (320, 64, False), (2048, 64, True), (1088, "h", False),
    (1024, "h", True), (1088, 64, False), (2048, 32, False), (320, 32, False)]


def consumer_plan(tile, tname):
    """four sub-cases per (tile, type) out of _CONSUMER_SPECS: over the three types a tile sees every h of HS (1, 2, 5, 16, 17 and 32 units), pairs of
    32-column slots, the single slot, exact and general statistics; M rotates through the ragged row counts (653 for the 320-row form), N2 through
    {128, 320}, the epilogue through 1, 2, 3.  The small-M kernel: 16 / 64 / h columns per slot, M in {1, 77}."""
    i, t = CONSUMER_TILES.index(tile), TYPES.index(tname)
    skinny = tile == -1
    Ms = [1, 77] if skinny else [653, 77, 203, 333] if tile == 320261 else [1, 77, 203, 333]
    out = []
    for k in range(4 * t, 4 * t + 4):
        h, sw, exact = _CONSUMER_SPECS[k]
        slotw = h if sw == "h" else ({64: 16, 32: 64}[sw] if skinny else sw)
        out.append(dict(M=Ms[(i + k) % len(Ms)], N2=[128, 320][(i + k) % 2], h=h, slotw=slotw, exact=exact, epi=1 + (i + k) % 3))
    return out


CHAIN = [(64128, 65064), (65128, 160128), (160256, 256259), (128064, 256261), (0, 0), (-1, -1)]     # tile1 x tile2 of the producer-into-consumer runs
