"""Shared numpy side of the value-edge tests of the exact index (not a test module): rows and queries at the ends of f32.

The f32 / f16 store holds only finite values of magnitude <= 1 (include/clip_amd.h, rules 1 - 4 of the index paragraph):

emulate_store   search_normalize_kernel in numpy f32: a row with a NaN or an infinity is the zero row; amax = m 2^e with m in [0.5, 1),
                y = x 2^-e (exact), then stored_queries of tests/test_gpu_search.py on y: the kernel's lane and butterfly order, the
                square root, the division and the rounding to the stored dtype.
unit64          x / |x|_2 in float64 (2^+-149 squared is far inside its range), the zero row for a non-finite or zero x.
bound_c         c(dim) of |stored_i - u_i| <= c 2^-24 |u_i|, in units of 2^-24 relative: the sum of squares rounds once per addition, a
                lane adds ceil(dim / 64) values and the butterfly six more, each square rounds once: (ceil(dim / 64) + 7) half-ulps on ss,
                halved by the square root: (ceil(dim / 64) + 7) / 2; the square root's own rounding, the division's and the first-order
                slack of the products of those factors: 1.5.
half_ulp16      half an fp16 ulp at a value, 2^-25 below 2^-14 (the subnormal spacing is 2^-24): what the f16 store adds.
case_rows       the rows of the scale tests with, for each, the row whose stored bits it must share.
write_index     an index file of the documented format from an array of stored values.
"""
import struct

import numpy as np

from test_gpu_search import NP_DT, stored_queries

DIMS = [4, 36, 64, 132, 512]      # part of one wave pass; no multiple of the k-step; one pass exactly; a partial third pass; eight passes
SCALES = [-100, -70, -60, -30, 30, 60, 100]
DT_CODE = {"f32": 0, "f16": 1, "i8": 3}
FILE_DT = {"f32": np.float32, "f16": np.float16, "i8": np.int8}
F32_MIN_NORMAL = 2.0 ** -126


def zeroed(x):
    """x (f32 [n, dim]) with every row that holds a NaN or an infinity replaced by the zero row: the twin the index must treat it as"""
    x = np.array(x, dtype=np.float32)
    x[~np.isfinite(x).all(axis=1)] = 0.0
    return x


def emulate_store(x, dtype):
    """what the index stores for the rows x, in the stored dtype ("f32" / "f16"), bit for bit"""
    x = zeroed(x)
    e = np.frexp(np.abs(x).max(axis=1))[1].astype(np.int32)          # 0 for the zero row
    y = np.ldexp(x, -e[:, None]).astype(np.float32)
    assert y.dtype == np.float32
    return stored_queries(y, dtype).astype(NP_DT[dtype])


def unit64(x):
    x = zeroed(x).astype(np.float64)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.where(n > 0, x / np.where(n > 0, n, 1.0), 0.0)


def bound_c(dim):
    return ((dim + 63) // 64 + 7) / 2.0 + 1.5


def half_ulp16(v):
    """half an fp16 ulp at |v| (float64 array): 2^(floor(log2 |v|) - 11), at least 2^-25"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    ex = np.where(v > 0, np.frexp(v)[1] - 1, -14)                     # floor(log2 |v|)
    return np.ldexp(1.0, np.maximum(ex, -14) - 11)


def store_error_ratio(stored, x, dtype):
    """max over the values of (|stored - u| - fp16 allowance) / (2^-24 |u|), u = unit64(x): to be <= bound_c(dim); rows of x whose unit
    vector has a zero stay out of the ratio and must be stored as exact zeros"""
    u = unit64(x)
    s = np.asarray(stored, dtype=np.float64)
    err = np.abs(s - u)
    if dtype == "f16":
        err = np.maximum(err - half_ulp16(np.maximum(np.abs(u), np.abs(s))), 0.0)
    nz = u != 0
    assert np.all(s[~nz] == 0)
    return float((err[nz] / (2.0 ** -24 * np.abs(u[nz]))).max()) if nz.any() else 0.0


def ordinary(rng, n, dim):
    """standard normal rows with every magnitude brought into [2^-8, 8]"""
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return (np.where(x < 0, -1.0, 1.0) * np.clip(np.abs(x), 2.0 ** -8, 8.0)).astype(np.float32)


def exactly_scaled(x, e):
    """x 2^e as f32 and whether that product is exact (every element finite and none lost bits to underflow)"""
    with np.errstate(over="ignore", under="ignore"):
        y = np.ldexp(x.astype(np.float32), e).astype(np.float32)
    exact = np.isfinite(y).all() and np.array_equal(y.astype(np.float64), np.ldexp(x.astype(np.float64), e))
    return y, bool(exact)


def case_rows(dim, n_base=8):
    """(rows f32 [n, dim], base int [n], kind str [n], e int [n]): row t must be stored with the bits of row base[t] (itself for a base
    row).  kind: "base" ordinary rows, magnitudes in [2^-8, 8]; "scaled" base rows times 2^e, e in SCALES; "sub" rows of subnormals
    (other ordinary rows times 2^-140, rounded to f32) and "up", each of them times 2^140 (exact), the base of its "sub" row; "wide" a
    base row with one element multiplied by 2^100 or by 2^-100, and "wide-scaled" those times 2^+-20 where that is exact."""
    rng = np.random.default_rng(4000 + dim)
    rows, base, kind, es = [], [], [], []

    def put(r, b, k, e):
        rows.append(np.asarray(r, dtype=np.float32))
        base.append(len(rows) - 1 if b is None else b)
        kind.append(k)
        es.append(e)
        return len(rows) - 1

    b0 = ordinary(rng, n_base, dim)
    ids = [put(r, None, "base", 0) for r in b0]
    for e in SCALES:
        for r, b in zip(b0, ids):
            y, exact = exactly_scaled(r, e)
            assert exact
            put(y, b, "scaled", e)
    with np.errstate(under="ignore"):
        sub = np.ldexp(ordinary(rng, n_base, dim), -140).astype(np.float32)
    for r in sub:
        y, exact = exactly_scaled(r, 140)
        assert exact and np.all(np.abs(r) < F32_MIN_NORMAL) and np.any(r != 0)
        put(r, put(y, None, "up", 0), "sub", -140)
    for t, r in enumerate(b0):
        for we in (100, -100):
            w, at = r.copy(), (5 * t + 3) % dim
            one, exact = exactly_scaled(r[at:at + 1], we)
            assert exact
            w[at] = one[0]
            b = put(w, None, "wide", 0)
            for e in (-20, 20):
                y, exact = exactly_scaled(w, e)
                if exact:
                    put(y, b, "wide-scaled", e)
    return np.stack(rows), np.array(base), np.array(kind), np.array(es)


def write_index(path, dim, dtype, values):
    """the documented file: "CLIPIDX1", u32 version 1, u32 dim, u32 dtype code, u64 n, then n rows of dim stored values, unpadded;
    values: an array of the file's dtype (f32, f16 or int8) or of raw bit patterns (uint32 / uint16 / uint8), [n, dim]"""
    v = np.ascontiguousarray(values)
    assert v.ndim == 2 and v.shape[1] == dim and v.dtype.itemsize == np.dtype(FILE_DT[dtype]).itemsize
    with open(path, "wb") as f:
        f.write(b"CLIPIDX1" + struct.pack("<IIIQ", 1, dim, DT_CODE[dtype], v.shape[0]))
        f.write(v.astype(v.dtype.newbyteorder("<"), copy=False).tobytes())


def read_index(path):
    """(dim, dtype name, stored values [n, dim] in the file's dtype) of an index file"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"CLIPIDX1"
    ver, dim, dt, n = struct.unpack("<IIIQ", raw[8:28])
    name = {c: k for k, c in DT_CODE.items()}[dt]
    assert ver == 1 and len(raw) == 28 + n * dim * np.dtype(FILE_DT[name]).itemsize
    return dim, name, np.frombuffer(raw, dtype=np.dtype(FILE_DT[name]).newbyteorder("<"), offset=28).reshape(n, dim).astype(FILE_DT[name])
