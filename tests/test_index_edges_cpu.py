"""CPU tier of the value-edge tests of the exact index: the numpy emulation of the normalising store (index_edges_common.emulate_store)
obeys the rules of include/clip_amd.h that tests/test_gpu_index_value_edges.py holds the kernel to, and the generated rows are what
those rules speak of.

1. non-finite input is the zero vector; 2. the stored bits do not depend on an exact power-of-two scale, subnormal rows included;
3. ordinary rows keep the bits of stored_queries (tests/test_gpu_search.py), the arithmetic without the scaling step; the float64 bound
|stored_i - u_i| <= c(dim) 2^-24 |u_i| (+ half an fp16 ulp for the f16 store) holds with room: the worst ratio is printed per dim."""
import numpy as np
import pytest

import index_edges_common as ie
from test_gpu_search import NP_DT, stored_queries


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", ie.DIMS)
def test_rule_1_non_finite_rows_are_zero_rows(dim, dtype):
    rng = np.random.default_rng(dim)
    x = ie.ordinary(rng, 12, dim)
    want = ie.emulate_store(x, dtype)
    for t, v in enumerate([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]):
        x[2 * t, [0, dim - 1, min(63, dim - 1), min(64, dim - 1), dim // 2, 1][t]] = v
    x[1] = np.nan
    x[3, 0], x[3, 1] = np.inf, np.nan
    got = ie.emulate_store(x, dtype)
    bad = ~np.isfinite(x).all(axis=1)
    assert bad.sum() == 8
    assert np.all(got[bad] == 0) and np.array_equal(bits(got[~bad]), bits(want[~bad])) and np.all(np.isfinite(got))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", ie.DIMS)
def test_rule_2_scaled_rows_share_their_base_rows_bits(dim, dtype):
    rows, base, kind, e = ie.case_rows(dim)
    got = ie.emulate_store(rows, dtype)
    assert np.array_equal(bits(got), bits(got[base]))
    assert np.all(np.abs(got.astype(np.float64)) <= 1) and np.all(np.abs(got[:, :].astype(np.float64)).max(axis=1) > 0)
    for k in ("base", "scaled", "sub", "up", "wide", "wide-scaled"):
        assert (kind == k).any(), k
    assert sorted(set(e[kind == "scaled"].tolist())) == ie.SCALES


@pytest.mark.parametrize("dim", ie.DIMS)
def test_generated_rows_are_exact_multiples_of_their_base_rows(dim):
    """the precondition of rule 2: row = base row times 2^e with every element finite and normal, or an exactly scaled subnormal"""
    rows, base, kind, e = ie.case_rows(dim)
    assert len(rows) <= 400 and np.all(np.isfinite(rows)) and np.all(rows != 0)
    for t in np.flatnonzero(base != np.arange(len(rows))):
        shift = int(e[t]) - int(e[base[t]])
        assert np.array_equal(rows[t].astype(np.float64), np.ldexp(rows[base[t]].astype(np.float64), shift)), (t, kind[t])
        if kind[t] != "sub":
            assert np.all(np.abs(rows[t]) >= ie.F32_MIN_NORMAL)
    ordinary = rows[kind == "base"]
    assert np.all((np.abs(ordinary) >= 2.0 ** -8) & (np.abs(ordinary) <= 8))
    assert np.all(np.abs(rows[kind == "sub"]) < ie.F32_MIN_NORMAL)
    wide = np.abs(rows[kind == "wide"].astype(np.float64))
    assert np.all(wide.max(axis=1) / wide.min(axis=1) >= 2.0 ** 89)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", ie.DIMS)
def test_rule_3_ordinary_rows_keep_the_bits_of_the_unscaled_arithmetic(dim, dtype):
    rng = np.random.default_rng(77 + dim)
    x = np.concatenate([ie.ordinary(rng, 200, dim), rng.standard_normal((200, dim)).astype(np.float32),
                        np.ldexp(ie.ordinary(rng, 50, dim), 20).astype(np.float32), np.ldexp(ie.ordinary(rng, 50, dim), -20).astype(np.float32)])
    x[5] = 0.0
    assert np.array_equal(bits(ie.emulate_store(x, dtype)), bits(stored_queries(x, dtype).astype(NP_DT[dtype])))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("dim", ie.DIMS)
def test_float64_bound_holds_for_the_emulation(dim, dtype):
    rng = np.random.default_rng(900 + dim)
    rows, base, kind, e = ie.case_rows(dim)
    x = np.concatenate([ie.ordinary(rng, 400, dim), rows])
    ratio = ie.store_error_ratio(ie.emulate_store(x, dtype), x, dtype)
    print("dim %d %s: worst |stored - u| / (2^-24 |u|) = %.2f of c = %.1f" % (dim, dtype, ratio, ie.bound_c(dim)))
    assert ratio <= ie.bound_c(dim)


def test_half_ulp16_and_file_round_trip(tmp_path):
    v = np.array([1.0, 0.75, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 0.0, 1.5 * 2.0 ** -3])
    assert ie.half_ulp16(v).tolist() == [2.0 ** -11, 2.0 ** -12, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -14]
    for dtype, a in (("f32", np.array([[1, 0, 0, -0.5]], np.float32)), ("f16", np.array([[1, 0, 0, -0.5]] * 3, np.float16)),
                     ("i8", np.array([[-128, 127, 0, 1]], np.int8))):
        p = str(tmp_path / (dtype + ".index"))
        ie.write_index(p, 4, dtype, a)
        dim, name, back = ie.read_index(p)
        assert (dim, name) == (4, dtype) and np.array_equal(back, a) and back.dtype == a.dtype
    ie.write_index(p, 4, "f16", np.array([[0x7e00, 0x3c00, 0, 0x3c01]], np.uint16))
    assert np.isnan(ie.read_index(p)[2][0, 0]) and ie.read_index(p)[2][0, 3] == np.float16(1 + 2.0 ** -10)
