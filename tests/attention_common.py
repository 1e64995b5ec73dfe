"""Shared pieces of the attention kernel tests (not a test module): ragged inputs with guard rows, the float64 definition of
softmax(Q K^T) V per (sequence, head) together with the sums the error bounds are made of, the two element-wise bounds (fp16 kernels of
k_attn.hip / k_attn_long.hip, f32 kernel of k_attn_f32.hip), numpy emulations of the kernels' arithmetic and planted errors that guard the
bounds themselves (test_attention_reference_cpu.py), the input sets of test_gpu_attention_ragged.py and the call of the C ABI hook.

fp16 bound.  Inputs are exact fp16, scores accumulate in f32, p = exp2(...) is rounded to fp16 once, the row sum is taken from the unrounded
f32 values and the output is rounded to fp16 once.  With e_k = exp(s_k - max) and p_k = e_k / sum(e):

    bound = 1.25 * [ 2^-11 * sum_k p_k |v_kd|  +  2^-11 * |want|  +  sum_{k : e_k < 2^-14} p_k |v_kd| ] + 1e-7

(half-ulp relative rounding of every p_k — also against the streaming kernel's running maximum, which is never above the final one, with the
rescale in f32; the output rounding; probabilities in the fp16 subnormal range may be lost entirely, so the bound does not depend on whether
the MFMA flushes subnormals; 1.25 covers the f32 second-order terms: score accumulation, hardware exp2, the reciprocal).

f32 bound: the worst-case forward error of the kernel as written, u = 2^-24, a_qk = sum_d |q_d k_kd|, x_k = max - s_k:

    bound = u * sum_k p_k (2 * d_head * a_qk + x_k + len + 16) |v_kd|  +  u * |want|

(the sequential FMA chain of a score, __expf's argument rounding, the len-term accumulations with their rescales)."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

SENTINEL = 777.0          # exact in fp16: a guard row of `out` survives the fp16 round trip of the hook bit for bit
GUARD = 128               # rows before seq_start[0] and after seq_start[nseq]: NaN in qkv, SENTINEL in out
HEAD_SIZES = (32, 64, 80, 88, 96, 104)
SCALES = (1, 6)           # the flat softmax of the uniform tests and a peaked one
F32_CHUNK = {32: 32, 64: 16, 80: 16, 88: 8, 96: 8, 104: 8}     # keys per LDS chunk of k_attn_f32.hip

TEXT_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 64, 76, 77]     # causal, d_head 64: max_len 77 / 80 (NT = 5), 112 (NT = 7, query-block pairs)
HEAD_LENS = [1, 16, 17, 47, 97, 160, 161, 257, 288]            # max_len 288: NT = 18
NT37_LENS = [1, 33, 300, 577, 592]                             # d_head 64, max_len 592
LONG_LENS = [1, 63, 64, 65, 129, 593, 700, 1025]               # past the whole-row kernel
WIDE_LENS = [[300, 1, 17, 64, 65, 128, 129, 200][i % 8] for i in range(44)]   # 44 * 2 heads * ceil(300 / 128) = 264 >= 256: 128-query workgroups
F32_LENS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130]           # around the chunk sizes 8 / 16 / 32 and the 64-query block

Ref = namedtuple("Ref", "want pabs psub pw32 inside")
Ref.__doc__ = """want f64 [rows, h]: the definition; pabs = sum_k p_k |v_kd|; psub = the same sum over keys with e_k < 2^-14;
pw32 = sum_k p_k (2 d_head a_qk + x_k + len + 16) |v_kd| (filled for unrounded inputs only: round_fp16 = False); inside bool [rows]: the row belongs to a sequence (every array is 0 elsewhere)."""


def h16(x):
    """round through fp16 (what the fp16 kernels' inputs are)"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def uniform_starts(nseq, T):
    return (np.arange(nseq + 1, dtype=np.int64) * T).astype(np.int32)


def make_ragged_qkv(lens, h, nh, scale, seed, guard=GUARD):
    """One batch: (qkv f32 [guard + sum(lens) + guard, 3h], seq_start int32 [nseq + 1]).  Values are standard normal times 0.7, the Q columns
    times scale / sqrt(d_head) (Q arrives pre-scaled).  In every sequence longer than 2 one query row r is replaced, in every head, by
    12 k_j / |k_j| for a random key j <= r (visible with and without the causal mask): key j dominates that row and the rest underflow
    fp16.  Guard rows are NaN."""
    dh = h // nh
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    body = (rng.standard_normal((n, 3 * h)) * 0.7).astype(np.float32)
    body[:, :h] *= np.float32(scale / np.sqrt(dh))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for i, ln in enumerate(lens):
        if ln <= 2:
            continue
        r = int(rng.integers(1, ln))
        j = int(rng.integers(0, r + 1))
        for hd in range(nh):
            kj = body[off[i] + j, h + hd * dh:h + (hd + 1) * dh].astype(np.float64)
            body[off[i] + r, hd * dh:(hd + 1) * dh] = (12.0 * kj / np.linalg.norm(kj)).astype(np.float32)
    qkv = np.full((n + 2 * guard, 3 * h), np.nan, dtype=np.float32)
    qkv[guard:guard + n] = body
    return qkv, (off + guard).astype(np.int32)


def _heads(seq_start, h, nh):
    """(sequence, first row, end row, head, head's columns) of a batch"""
    dh = h // nh
    for i in range(len(seq_start) - 1):
        for hd in range(nh):
            yield i, int(seq_start[i]), int(seq_start[i + 1]), hd, slice(hd * dh, (hd + 1) * dh)


def _visible(n, causal):
    return np.tril(np.ones((n, n), dtype=bool)) if causal else np.ones((n, n), dtype=bool)


PLANTS = ("causal_off_by_one", "pad_unmasked", "drop_key", "neighbour_v")


def attention_ref_ragged(qkv, seq_start, h, nh, causal, round_fp16, plant=None):
    """softmax(Q K^T) V in float64, one (sequence, head) at a time, on the inputs as they are or rounded to fp16 first: a Ref.
    plant (test_attention_reference_cpu.py: what the bounds must reject) computes a wrong `want` instead, still in float64:
      causal_off_by_one  the last visible key min(q, len - 1) of every query but query 0 is masked (`key < kmax`)
      pad_unmasked       the zero padded keys len .. 16 * ceil(len / 16) - 1 (score 0, V = 0) take part in the softmax
      drop_key           key len / 2 is masked for every query (sequences of 2 and more)
      neighbour_v        V of key len / 2 is read from the first row of the next sequence (cyclic)"""
    assert plant is None or plant in PLANTS
    seq_start = np.asarray(seq_start)
    x = (h16(qkv) if round_fp16 else np.asarray(qkv, dtype=np.float32)).astype(np.float64)
    rows, dh = x.shape[0], h // nh
    want, pabs, psub, pw32 = (np.zeros((rows, h)) for _ in range(4))
    inside = np.zeros(rows, dtype=bool)
    nseq = len(seq_start) - 1
    for i, r0, r1, hd, cols in _heads(seq_start, h, nh):
        n = r1 - r0
        inside[r0:r1] = True
        q, k, v = x[r0:r1, cols], x[r0:r1, h + hd * dh:h + (hd + 1) * dh], x[r0:r1, 2 * h + hd * dh:2 * h + (hd + 1) * dh]
        vis = _visible(n, causal)
        if plant == "causal_off_by_one":
            kmax = np.minimum(np.arange(n), n - 1) if causal else np.full(n, n - 1)
            vis = np.arange(n)[None, :] < kmax[:, None]
            vis[0, 0] = True        # (a query that sees nothing is NaN: let the bound reject the plant by its values)
        elif plant == "drop_key" and n >= 2:
            vis = vis.copy()
            vis[:, n // 2] = False
        elif plant == "neighbour_v":
            v = v.copy()
            v[n // 2] = x[int(seq_start[(i + 1) % nseq]), 2 * h + hd * dh:2 * h + (hd + 1) * dh]
        elif plant == "pad_unmasked":
            pad = -n % 16
            k = np.concatenate([k, np.zeros((pad, dh))])
            v = np.concatenate([v, np.zeros((pad, dh))])
            vis = np.concatenate([vis, np.ones((n, pad), dtype=bool)], axis=1)
        with np.errstate(invalid="ignore"):
            s = np.where(vis, q @ k.T, -np.inf)
            xk = s.max(1, keepdims=True) - s                     # max - s_k; +inf for masked keys
            e = np.exp(-xk)
            p = e / e.sum(1, keepdims=True)
        av = np.abs(v)
        want[r0:r1, cols] = p @ v
        if plant is None:
            pabs[r0:r1, cols] = p @ av
            psub[r0:r1, cols] = np.where(e < 2.0 ** -14, p, 0.0) @ av
            if not round_fp16:      # (the f32 bound's sum: the f32 kernel takes its inputs as they are)
                a = np.abs(q) @ np.abs(k).T
                pw32[r0:r1, cols] = (p * (2 * dh * a + np.where(vis, xk, 0.0) + n + 16)) @ av
    return Ref(want, pabs, psub, pw32, inside)


def fp16_bound(ref):
    return 1.25 * (2.0 ** -11 * ref.pabs + 2.0 ** -11 * np.abs(ref.want) + ref.psub) + 1e-7


def f32_bound(ref):
    assert ref.pw32.any(), "the f32 bound belongs to a reference on unrounded inputs"
    return 2.0 ** -24 * ref.pw32 + 2.0 ** -24 * np.abs(ref.want)


def err_over_bound(got, ref, bound):
    """max over the rows inside sequences of |got - want| / bound; inf if a value there is not finite"""
    g = np.asarray(got, dtype=np.float64)[ref.inside]
    if not np.all(np.isfinite(g)):
        return np.inf
    return float((np.abs(g - ref.want[ref.inside]) / bound[ref.inside]).max())


def ulps_at_row_scale(a, b, h, nh):
    """|a - b| in fp16 ulps of the largest magnitude of the (query, head) row it belongs to: the two kernels round different fp16
    probabilities (the streaming one against the running maximum), so an output that nearly cancels can differ by many ulps of its own."""
    dh = h // nh
    a3, b3 = a.reshape(-1, nh, dh), b.reshape(-1, nh, dh)
    scale = np.maximum(np.abs(a3).max(-1, keepdims=True), np.abs(b3).max(-1, keepdims=True))
    ulp = np.spacing(scale.astype(np.float16)).astype(np.float32)
    return (np.abs(a3 - b3) / ulp).max()


# ---- numpy emulations of the kernels' arithmetic (they guard the bounds; the GPU tests never use them as a reference) ----
L2E = np.float32(1.44269504088896340736)


def _to_fp16(e, flush):
    e16 = e.astype(np.float16)
    if flush:
        e16 = np.where(np.abs(e16) < np.float16(2.0 ** -14), np.float16(0), e16)
    return e16.astype(np.float32)


def emulate_fp16(qkv, seq_start, h, nh, causal, flush, chunk=None):
    """The fp16 kernels' arithmetic: fp16 inputs, f32 scores, e = exp2(s * log2(e) - max * log2(e)) in f32, the row sum from the f32 values,
    e rounded to fp16 (flush: subnormal results become 0) times V accumulated in f32, one reciprocal, the output rounded to fp16.
    chunk = None: the whole-row kernel (one maximum per row).  chunk = 64: the streaming kernel (every chunk of keys is rounded against the
    running maximum, earlier sums and outputs are rescaled in f32)."""
    x = h16(qkv)
    out = np.zeros((x.shape[0], h), dtype=np.float32)
    dh = h // nh
    for _, r0, r1, hd, cols in _heads(seq_start, h, nh):
        n = r1 - r0
        q, k, v = x[r0:r1, cols], x[r0:r1, h + hd * dh:h + (hd + 1) * dh], x[r0:r1, 2 * h + hd * dh:2 * h + (hd + 1) * dh]
        s = np.where(_visible(n, causal), q @ k.T, np.float32(-np.inf)).astype(np.float32)
        step = n if chunk is None else chunk
        m = np.full((n, 1), -np.inf, dtype=np.float32)
        ls = np.zeros((n, 1), dtype=np.float32)
        o = np.zeros((n, dh), dtype=np.float32)
        for k0 in range(0, n, step):
            sc_ = s[:, k0:k0 + step]
            mn = np.maximum(m, sc_.max(1, keepdims=True))
            with np.errstate(invalid="ignore"):
                sc = np.exp2((m - mn) * L2E).astype(np.float32)          # first chunk: exp2(-inf) = 0
                e = np.exp2((sc_.astype(np.float64) * L2E + (-mn * L2E).astype(np.float64)).astype(np.float32)).astype(np.float32)   # one fma
            m = mn
            ls = ls * sc + e.sum(1, keepdims=True, dtype=np.float32)
            o = o * sc + _to_fp16(e, flush) @ v[k0:k0 + step]
        out[r0:r1, cols] = (o * (np.float32(1) / ls)).astype(np.float16).astype(np.float32)
    return out


def emulate_f32(qkv, seq_start, h, nh, causal):
    """k_attn_f32.hip's arithmetic: every score one sequential f32 FMA chain over d, online softmax over chunks of F32_CHUNK[d_head] keys
    with f32 exp, the sum and the output row accumulated key by key in f32, one reciprocal."""
    x = np.asarray(qkv, dtype=np.float32)
    out = np.zeros((x.shape[0], h), dtype=np.float32)
    dh = h // nh
    kc = F32_CHUNK[dh]
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    for _, r0, r1, hd, cols in _heads(seq_start, h, nh):
        n = r1 - r0
        q, k, v = x[r0:r1, cols], x[r0:r1, h + hd * dh:h + (hd + 1) * dh], x[r0:r1, 2 * h + hd * dh:2 * h + (hd + 1) * dh]
        s = np.zeros((n, n), dtype=np.float32)
        for d in range(dh):
            s = fma(q[:, d:d + 1], k[None, :, d], s)
        s = np.where(_visible(n, causal), s, np.float32(-np.inf))
        m = np.full((n, 1), -np.inf, dtype=np.float32)
        sm = np.zeros((n, 1), dtype=np.float32)
        o = np.zeros((n, dh), dtype=np.float32)
        for k0 in range(0, n, kc):
            mn = np.maximum(m, s[:, k0:k0 + kc].max(1, keepdims=True))
            with np.errstate(invalid="ignore"):
                sc = np.exp(m - mn).astype(np.float32)
            m = mn
            sm = sm * sc
            o = o * sc
            p = np.exp(s[:, k0:k0 + kc] - mn).astype(np.float32)
            for j in range(p.shape[1]):
                sm = sm + p[:, j:j + 1]
            for j in range(p.shape[1]):
                o = fma(p[:, j:j + 1], v[None, k0 + j], o)
        out[r0:r1, cols] = o * (np.float32(1) / sm)
    return out


# ---- the input sets of the GPU tests, built once per process and never written again ----
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


BATCH_LENS = {"text": TEXT_LENS, "heads": HEAD_LENS, "heads4": HEAD_LENS * 4, "nt37": NT37_LENS, "long": LONG_LENS, "wide": WIDE_LENS,
              "f32": F32_LENS, "uniform65": [65, 65, 65]}


@functools.lru_cache(maxsize=None)
def batch(name, dh, scale):
    """(qkv, seq_start, h, n_head) of a named input set: two heads of dh, seeded by (name, dh, scale).  "uniform65" has no guard rows (it
    is run through seq_start == NULL)."""
    lens = BATCH_LENS[name]
    seed = 1000 * sorted(BATCH_LENS).index(name) + 10 * dh + scale
    qkv, ss = make_ragged_qkv(lens, 2 * dh, 2, scale, seed, guard=0 if name == "uniform65" else GUARD)
    return _frozen(qkv, ss) + (2 * dh, 2)


@functools.lru_cache(maxsize=16)      # (a test and its neighbours share one; the whole list would be a gigabyte)
def reference(name, dh, scale, causal, round_fp16):
    qkv, ss, h, nh = batch(name, dh, scale)
    ref = attention_ref_ragged(qkv, ss, h, nh, causal, round_fp16)
    _frozen(*ref)
    return ref


def fp16_sets():
    """(name, d_head, causal) of every input set the fp16 kernels run in test_gpu_attention_ragged.py (each at both SCALES)"""
    sets = [("text", 64, 1)]
    sets += [(n, dh, c) for n in ("heads", "heads4") for dh in HEAD_SIZES for c in (0, 1)]
    sets += [("nt37", 64, c) for c in (0, 1)]
    sets += [("long", dh, c) for dh in (64, 104) for c in (0, 1)]
    sets += [("wide", 64, c) for c in (0, 1)]
    return sets


def f32_sets():
    """... and of the f32 kernel ("text" and "heads" are its batches of the independence test)"""
    sets = [(n, dh, c) for n in ("f32", "uniform65", "heads") for dh in HEAD_SIZES for c in (0, 1)]
    return sets + [("text", 64, 1)]


# ---- the hook ----
def run_ragged(L, qkv, seq_start, max_len, h, nh, causal, kernel, nseq=None):
    """clip_amd_test_attention_ragged on a batch: (rc, out) with out [rows_total, h] f32, SENTINEL wherever nothing was written.
    seq_start None: nseq uniform sequences of max_len rows."""
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    out = np.full((qkv.shape[0], h), SENTINEL, dtype=np.float32)
    if seq_start is None:
        ssp = None
    else:
        ss = np.ascontiguousarray(seq_start, dtype=np.int32)
        ssp, nseq = ss.ctypes.data_as(C.POINTER(C.c_int32)), len(ss) - 1
    rc = L.clip_amd_test_attention_ragged(qkv.ctypes.data_as(C.POINTER(C.c_float)), qkv.shape[0], ssp, nseq, max_len, h, nh, causal,
                                          out.ctypes.data_as(C.POINTER(C.c_float)), kernel)
    return rc, out
