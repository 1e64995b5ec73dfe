"""GPU tier, kernel level: the memory-bound kernels at the two ends of each tower (k_misc.hip, row_stats_kernel of k_skinny.hip) through the
C ABI test hooks of include/clip_amd.h — text embedding, im2col, LayerNorm and its fold-entry form, class-token rows, row gather, L2
normalisation, row statistics, dtype conversion.  Seeded numpy inputs, no model files.

Most of these kernels are copies, fp16 roundings and f32 expressions of two roundings, and the library is built with -ffp-contract=off, so the
tests ask for BITS wherever the value can be predicted and for a derived rounding bound elsewhere (u = 2^-24 is the unit roundoff of f32,
gamma(k) = k u / (1 - k u) the usual bound on k accumulated roundings).  The hooks fill their output buffers with a poison pattern before
the launch (f32: quiet NaN 0x7fc00000, fp16: 0x7e00), so "the kernel did not write here" is a check on bits as well.
Attention and the GEMMs are in test_gpu_kernels.py / test_gpu_long_attention.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
POISON32, POISON16 = 0x7fc00000, 0x7e00
TYPES = ["f32", "f16", "q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
BLOCK_BYTES = {"q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "q8_0": 34}
EPS = 1e-5


@pytest.fixture(scope="module")
def L(clip_lib):
    if clip_lib.device_count() < 1:
        pytest.fail("GPU tier needs a HIP device: the product has no CPU fallback")
    return clip_lib.lib()


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _u16p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint16))


def _i32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def gamma(k):
    return k * U / (1 - k * U)


def nv_of(h):
    """float4 per lane of the instantiation that the launchers pick for a row of h floats."""
    return 1 if h <= 256 else 2 if h <= 512 else 3 if h <= 768 else 4 if h <= 1024 else 5 if h <= 1280 else 8


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits16(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def assert_bits_equal(got, want, what):
    """got, want: integer arrays of bit patterns (or float arrays of one dtype, compared by their bits)."""
    if got.dtype.kind == "f":
        got, want = got.view("u%d" % got.itemsize), np.ascontiguousarray(want, dtype=got.dtype).view("u%d" % got.itemsize)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d elements differ, first at %s: got 0x%x want 0x%x" % (
        what, len(bad), got.size, bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def assert_poison(a, what):
    if a.dtype == np.uint16:
        assert_bits_equal(a, np.full(a.shape, POISON16, dtype=np.uint16), what + " (must stay unwritten)")
    else:
        assert_bits_equal(bits32(a), np.full(a.shape, POISON32, dtype=np.uint32), what + " (must stay unwritten)")


def nan32(shape):
    return np.full(shape, np.nan, dtype=np.float32)


def rows_data(rng, rows, h, ld=None):
    """[rows][ld] f32, every row with its own mean and scale (a row read from the wrong place is a gross error); columns >= h hold NaN."""
    ld = ld or h
    x = nan32((rows, ld))
    mean = rng.uniform(-3, 3, size=(rows, 1))
    scale = rng.uniform(0.5, 4, size=(rows, 1))
    x[:, :h] = (rng.standard_normal((rows, h)) * scale + mean).astype(np.float32)
    return x


def ln_params(rng, h):
    return (1 + rng.standard_normal(h) * 0.05).astype(np.float32), (rng.standard_normal(h) * 0.05).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# fold entry (row_fold_prep): shared by the text embedding and LayerNorm-prep tests
# --------------------------------------------------------------------------------------------------------------------------------
def check_fold(y, g, h, centred, xg, stats, mu, what):
    """What row_fold_prep leaves for the rows y [rows][h] (the kernel's own f32 output, which the caller has pinned by an independent reference).

    mu (centred form) = f32(s) / f32(h): one correctly rounded division of the kernel's own sum, so bitwise.  xg = f16(f32(f32(y - off) g)),
    off = mu or 0: two f32 roundings and one conversion, each predictable in numpy f32, so bitwise.  s and q are sums in an order the test does
    not replicate: one element passes through at most 4 NV lane additions and 6 shuffle levels, so against float64 sums of the same y
        |s - S| <= (4 NV + 8) u sum|y|,     |q - Q| <= (4 NV + 12) u sum (y - mean)^2
    (the second with the two roundings of forming and squaring the deviation).  The kernel takes its deviations about its own f32 mean m, not
    the exact one: sum (y - m)^2 = Q + h (m - mean)^2, and the extra term is of order u^2 sum|y|^2 / h: below 1e-6 of the bound for these rows."""
    rows = y.shape[0]
    nv = nv_of(h)
    y64 = y.astype(np.float64)
    s, q = stats[:, 0], stats[:, 1]
    S = y64.sum(1)
    Q = ((y64 - S[:, None] / h) ** 2).sum(1)
    es, eq = np.abs(s - S), np.abs(q - Q)
    bs, bq = (4 * nv + 8) * U * np.abs(y64).sum(1), (4 * nv + 12) * U * Q
    print("%s: max |s-S|/bound %.3f  max |q-Q|/bound %.3f" % (what, (es / bs).max(), (eq / bq).max()))
    assert (es <= bs).all(), "%s: sum off by %g of its bound at row %d" % (what, (es / bs).max(), int((es / bs).argmax()))
    assert (eq <= bq).all(), "%s: sum of squared deviations off by %g of its bound at row %d" % (what, (eq / bq).max(), int((eq / bq).argmax()))
    if centred:
        want_mu = s.astype(np.float32) / np.float32(h)
        assert_bits_equal(mu, want_mu, what + " mu")
        off = mu.reshape(rows, 1)
    else:
        assert_poison(mu, what + " mu of the uncentred form")
        off = np.zeros((rows, 1), dtype=np.float32)
    d = y - off
    assert d.dtype == np.float32
    want_xg = (d * g[None, :]).astype(np.float16)
    assert_bits_equal(xg[:, :h], bits16(want_xg), what + " xg")
    assert_poison(xg[:, h:], what + " xg padding")


# --------------------------------------------------------------------------------------------------------------------------------
# text embedding
# --------------------------------------------------------------------------------------------------------------------------------
def _f16_scales(rng, shape, lo, hi):
    """finite fp16 of both signs, as raw bytes [..., 2]."""
    v = (rng.uniform(lo, hi, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float16)
    assert np.isfinite(v).all() and (v > 0).any() and (v < 0).any()
    return v.view(np.uint8).reshape(shape + (2,))


def raw_table(rng, tname, vocab, h):
    """a [vocab][h] embedding table in the ggml layout of `tname`, built from random bytes (not through the quantiser: every code occurs)."""
    if tname == "f32":
        return (rng.standard_normal((vocab, h)) * 0.3).astype(np.float32).view(np.uint8).reshape(vocab, -1)
    if tname == "f16":
        return (rng.standard_normal((vocab, h)) * 0.3).astype(np.float16).view(np.uint8).reshape(vocab, -1)
    nb = h // 32
    parts = [_f16_scales(rng, (vocab, nb), 0.004, 0.05)]
    if tname in ("q4_1", "q5_1"):
        parts.append(_f16_scales(rng, (vocab, nb), 0.01, 0.5))
    if tname in ("q5_0", "q5_1"):
        qh = rng.integers(0, 256, size=(vocab, nb, 4), dtype=np.uint8)
        qh[0, 0], qh[0, 1] = (0, 0, 0, 0x80), (0xff, 0xff, 0xff, 0x7f)      # bit 31 alone set / alone clear
        word = qh.view(np.uint32)
        for bit in range(32):
            got = (word >> np.uint32(bit)) & np.uint32(1)
            assert got.any() and not got.all(), "qh bit %d must occur set and clear" % bit
        parts.append(qh)
    qs = rng.integers(0, 256, size=(vocab, nb, 32 if tname == "q8_0" else 16), dtype=np.uint8)
    if tname == "q8_0":
        qs[0, 0, :4], qs[1, 0, 28:] = (0x80, 0x7f, 0x80, 0x7f), (0x7f, 0x80, 0x7f, 0x80)       # -128 and 127
        assert (qs == 0x80).any() and (qs == 0x7f).any()
    else:
        assert set(np.unique(qs & 15)) == set(range(16)) and set(np.unique(qs >> 4)) == set(range(16))
    parts.append(qs)
    raw = np.ascontiguousarray(np.concatenate(parts, axis=2))
    assert raw.shape == (vocab, nb, BLOCK_BYTES[tname])
    return raw.reshape(vocab, -1)


def np_dequant(tname, raw, vocab, h):
    """the ggml block formats in plain numpy f32: q d (+ m), element j of a block from the low nibble of byte j (j < 16) or the high nibble of
    byte j - 16, the fifth bit of q5 from bit j of qh."""
    if tname == "f32":
        return raw.view(np.float32).reshape(vocab, h).copy()
    if tname == "f16":
        return raw.view(np.float16).reshape(vocab, h).astype(np.float32)
    nb = h // 32
    blk = raw.reshape(vocab, nb, BLOCK_BYTES[tname])
    f16_at = lambda o: np.ascontiguousarray(blk[:, :, o:o + 2]).view(np.float16).astype(np.float32)       # [vocab][nb][1]
    d = f16_at(0)
    if tname == "q8_0":
        return (np.ascontiguousarray(blk[:, :, 2:]).view(np.int8).astype(np.float32) * d).reshape(vocab, h)
    has_m, has_h = tname in ("q4_1", "q5_1"), tname in ("q5_0", "q5_1")
    o = 4 if has_m else 2
    q = None
    if has_h:
        qh = np.ascontiguousarray(blk[:, :, o:o + 4]).view(np.uint32)                  # [vocab][nb][1]
        hi = ((qh >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(np.int32)     # [vocab][nb][32]
        o += 4
    qs = blk[:, :, o:]
    q = np.concatenate([qs & 15, qs >> 4], axis=2).astype(np.int32)
    if has_h:
        q = q | (hi << 4)
    if has_m:
        return (q.astype(np.float32) * d + f16_at(2)).reshape(vocab, h)
    return ((q - (16 if has_h else 8)).astype(np.float32) * d).reshape(vocab, h)


def ragged(rng, nseq, n_pos):
    """nseq sequence lengths >= 1: mostly 1, one of n_pos, a total that is no multiple of 4; -> seq_start [nseq + 1]."""
    lens = np.where(rng.random(nseq) < 0.8, 1, rng.integers(2, n_pos, size=nseq))
    lens[rng.integers(0, nseq)] = n_pos
    if nseq > 1 and lens.sum() % 4 == 0:
        i = int(np.argmax(lens < n_pos - 1))
        lens[i] += 1
    assert lens.min() >= 1 and lens.max() == n_pos and (nseq < 63 or (lens == 1).sum() >= nseq // 2)
    assert lens.sum() % 4 != 0
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def run_text_embed(L, tname, raw, h, ids, seq, pos, g, centred):
    rows, nseq, ldxg = len(ids), len(seq) - 1, h + 4
    x, xg, stats, mu = np.empty((rows, h), np.float32), np.empty((rows, ldxg), np.uint16), np.empty((rows, 2), np.float32), np.empty(rows, np.float32)
    rc = L.clip_amd_test_text_embed(ref.GGML_TYPES[tname], _vp(raw), raw.size, h, _i32p(ids), _i32p(seq), nseq, rows, _fp(pos), pos.shape[0],
                                    _fp(g), int(centred), _fp(x), _u16p(xg), ldxg, _fp(stats), _fp(mu))
    assert rc == 0, "clip_amd_test_text_embed rc=%d" % rc
    return x, xg, stats, mu


def check_text_embed(L, tname, h, nseq, seed, modes):
    """x[r] = dequant(table[ids[r]]) + pos[r - start of r's sequence], required BITWISE: for the block formats q d is exact in f32 (q has at most
    8 significant bits, the fp16 scale 11), + m is one rounding and + pos one more — the same two roundings numpy f32 makes; for f16 / f32
    tables the widening is exact and + pos is the only rounding.  The dequantised table itself comes from the oracle's ggml code
    (ref.dequantize) and from np_dequant above, which must agree bitwise before either is used."""
    rng = np.random.default_rng(seed)
    vocab, n_pos = 97, 77
    raw = raw_table(rng, tname, vocab, h)
    table = np_dequant(tname, raw, vocab, h)
    assert table.dtype == np.float32
    assert_bits_equal(table, ref.dequantize(ref.GGML_TYPES[tname], raw.reshape(-1), vocab, h), "np_dequant against the oracle's ggml dequantiser")
    seq = ragged(rng, nseq, n_pos)
    rows = int(seq[-1])
    ids = rng.integers(0, vocab, size=rows).astype(np.int32)
    ids[:vocab] = rng.permutation(vocab)[:min(rows, vocab)]
    pos = (rng.standard_normal((n_pos, h)) * 0.1).astype(np.float32)
    t = np.arange(rows) - np.repeat(seq[:-1], np.diff(seq))
    want = table[ids] + pos[t]
    assert want.dtype == np.float32
    g = (1 + rng.standard_normal(h) * 0.1).astype(np.float32)
    for mode in modes:
        what = "text_embed %s h=%d nseq=%d rows=%d %s" % (tname, h, nseq, rows, mode)
        x, xg, stats, mu = run_text_embed(L, tname, raw, h, ids, seq, pos, None if mode == "plain" else g, mode == "centred")
        assert_bits_equal(x, want, what + " x")
        if mode == "plain":
            assert_poison(xg, what + " xg")
            assert_poison(stats, what + " stats")
            assert_poison(mu, what + " mu")
        else:
            check_fold(x, g, h, mode == "centred", xg, stats, mu, what)


@pytest.mark.parametrize("h", [64, 320, 768, 1024, 1280, 1344, 2048])
@pytest.mark.parametrize("tname", TYPES)
def test_text_embed(L, tname, h):
    """Every table format at every instantiation (NV = 1, 2, 3, 4, 5, 8, 8), plain and as the fold entry, centred and not; the argument for
    bitwise equality is check_text_embed's, the bounds on the statistics check_fold's."""
    check_text_embed(L, tname, h, 5, 1000 * h + TYPES.index(tname), ["plain", "uncentred", "centred"])


SEARCH_TYPES = {1: "q5_1", 2: "q8_0", 63: "q4_0", 64: "q5_0", 65: "q4_1", 66: "f16", 4096: "q5_1", 4097: "f32"}


@pytest.mark.parametrize("nseq", sorted(SEARCH_TYPES))
def test_text_embed_sequence_search(L, nseq):
    """The 64-ary search of seq_start at the sequence counts where its step changes (one probe round up to 64 sequences, two up to 4096, three
    beyond): the position row of every token, so a search that is off by one at one boundary breaks bitwise equality of that row."""
    check_text_embed(L, SEARCH_TYPES[nseq], 64, nseq, 77 + nseq, ["plain", "centred"])


# --------------------------------------------------------------------------------------------------------------------------------
# im2col
# --------------------------------------------------------------------------------------------------------------------------------
def tie_pixels(rng, shape):
    """f32 values of which a quarter each are: arbitrary, exactly half way between two neighbouring fp16 values (a tie of the rounding), the next
    f32 above such a tie, the next f32 below."""
    with np.errstate(over="ignore"):
        v = rng.standard_normal(shape).astype(np.float32)
        lo = v.astype(np.float16)
        hi = np.nextafter(lo, np.float16(np.inf))
        tie = (lo.astype(np.float32) + hi.astype(np.float32)) * np.float32(0.5)      # exact: 12 significant bits
        assert ((tie.astype(np.float64) * 2) == lo.astype(np.float64) + hi.astype(np.float64)).all()
        kind = rng.integers(0, 4, size=shape)
        out = np.where(kind == 0, v, np.where(kind == 1, tie, np.where(kind == 2, np.nextafter(tie, np.float32(np.inf)),
                                                                      np.nextafter(tie, np.float32(-np.inf))))).astype(np.float32)
    return out


@pytest.mark.parametrize("S,P,Kpad", [(64, 32, 3072), (32, 8, 192), (64, 16, 768), (28, 14, 640), (21, 7, 192), (16, 4, 64)])
def test_im2col(L, S, P, Kpad):
    """col[(b, oy, ox)][(c, ky, kx)] = fp16(img[b][oy P + ky][ox P + kx][c]): a gather and one round-to-nearest-even conversion, which numpy's
    astype(float16) makes too, so BITWISE; K padding columns are +0.  The first three shapes (even P, Kpad = 3 P P) run the pixel-pair kernel,
    the others the scalar one.  The fp16-input form (images rounded by launch_f32_to_f16 first) must give the same bits: rounding twice to the
    same format is rounding once."""
    rng = np.random.default_rng(S * 1000 + P)
    B, G, K = 3, S // P, 3 * P * P
    imgs = tie_pixels(rng, (B, S, S, 3))
    want = np.zeros((B * G * G, Kpad), dtype=np.float16)
    want[:, :K] = imgs.reshape(B, G, P, G, P, 3).transpose(0, 1, 3, 5, 2, 4).reshape(B * G * G, K).astype(np.float16)
    cols = []
    for f16 in (0, 1):
        col = np.empty((B * G * G, Kpad), np.uint16)
        rc = L.clip_amd_test_im2col(_fp(imgs), f16, B, S, P, Kpad, _u16p(col))
        assert rc == 0, "clip_amd_test_im2col rc=%d" % rc
        assert_bits_equal(col, bits16(want), "im2col S=%d P=%d Kpad=%d %s input" % (S, P, Kpad, "fp16" if f16 else "f32"))
        assert (col[:, K:] == 0).all(), "K padding must be +0"
        cols.append(col)
    assert_bits_equal(cols[1], cols[0], "fp16-input against f32-input im2col")


# --------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------------------------------------------------
def run_ln(L, x, w, b, rows, h, in_rows=None, in_row_mul=1, want16=True, want32=True):
    """-> (out16 bits [rows][h + 12], out32 [rows][h + 8]) of ONE launch, padding included."""
    ld16, ld32 = h + 12, h + 8
    o16 = np.empty((rows, ld16), np.uint16) if want16 else None
    o32 = np.empty((rows, ld32), np.float32) if want32 else None
    rc = L.clip_amd_test_layernorm_ex(_fp(x), x.shape[0], x.shape[1], _i32p(in_rows), in_row_mul, _fp(w), _fp(b), EPS, rows, h, _u16p(o16), ld16, _fp(o32), ld32)
    assert rc == 0, "clip_amd_test_layernorm_ex rc=%d" % rc
    return o16, o32


def check_ln(o16, o32, src, w, b, h, what):
    """out32 against the oracle (atol 2e-5, rtol 1e-5: the bounds test_gpu_kernels.py uses for this kernel); out16 = fp16 of the SAME f32 value
    (one conversion of the value the launch also stored), so bitwise against out32 of the same launch; the padding of both stays poisoned."""
    want = ref.layer_norm(np.ascontiguousarray(src[:, :h]), w, b, EPS)
    np.testing.assert_allclose(o32[:, :h], want, atol=2e-5, rtol=1e-5, err_msg=what)
    assert_poison(o32[:, h:], what + " out32 padding")
    assert_bits_equal(o16[:, :h], bits16(o32[:, :h].astype(np.float16)), what + " out16 against out32 of the same launch")
    assert_poison(o16[:, h:], what + " out16 padding")


LN_SHAPES = [(r, h) for r in (1, 5, 4095, 4096, 4097) for h in (64, 192)] + [(37, h) for h in (64, 192, 512, 768, 1024, 1280, 1344, 2048)]


@pytest.mark.parametrize("rows,h", LN_SHAPES)
def test_layernorm(L, rows, h):
    """Padded leading dimensions on the input (ldx = h + 4, the padding holds NaN) and both outputs; from 4096 rows the launcher runs two rows
    per wave, below it one: both forms do the same arithmetic per row, so the rows of a large launch must equal BITWISE the same rows run in two
    launches below the threshold (this also covers the odd last row of 4097, whose wave has no second row)."""
    rng = np.random.default_rng(rows * 4099 + h)
    x = rows_data(rng, rows, h, h + 4)
    w, b = ln_params(rng, h)
    what = "layernorm rows=%d h=%d" % (rows, h)
    o16, o32 = run_ln(L, x, w, b, rows, h)
    check_ln(o16, o32, x, w, b, h, what)
    only16, _ = run_ln(L, x, w, b, rows, h, want32=False)
    _, only32 = run_ln(L, x, w, b, rows, h, want16=False)
    assert_bits_equal(only16, o16, what + " out16 alone")
    assert_bits_equal(only32, o32, what + " out32 alone")
    if rows >= 4096:
        cut = rows // 2 + 1
        assert cut < 4096 and rows - cut < 4096
        a16, a32 = run_ln(L, np.ascontiguousarray(x[:cut]), w, b, cut, h)
        b16, b32 = run_ln(L, np.ascontiguousarray(x[cut:]), w, b, rows - cut, h)
        assert_bits_equal(o32, np.concatenate([a32, b32]), what + " two rows per wave against one row per wave, out32")
        assert_bits_equal(o16, np.concatenate([a16, b16]), what + " two rows per wave against one row per wave, out16")


@pytest.mark.parametrize("rows,n_src,h", [(37, 50, 192), (37, 50, 1344), (4099, 300, 64)])
def test_layernorm_in_rows(L, rows, n_src, h):
    """in_rows: a selection with repeats and omissions, in both forms (one and two rows per wave)."""
    rng = np.random.default_rng(rows + h)
    x = rows_data(rng, n_src, h, h + 4)
    w, b = ln_params(rng, h)
    in_rows = rng.integers(0, n_src, size=rows).astype(np.int32)
    in_rows[-1] = n_src - 1
    assert len(set(in_rows.tolist())) < rows
    o16, o32 = run_ln(L, x, w, b, rows, h, in_rows=in_rows)
    check_ln(o16, o32, x[in_rows], w, b, h, "layernorm in_rows rows=%d h=%d" % (rows, h))


@pytest.mark.parametrize("B,T,h", [(9, 5, 192), (7, 50, 768), (4100, 3, 64)])
def test_layernorm_in_row_mul(L, B, T, h):
    """in_row_mul = T on a [B T][h] input: the pooled tail's class-token rows b T."""
    rng = np.random.default_rng(B + T + h)
    x = rows_data(rng, B * T, h, h + 4)
    w, b = ln_params(rng, h)
    o16, o32 = run_ln(L, x, w, b, B, h, in_row_mul=T)
    check_ln(o16, o32, x[::T], w, b, h, "layernorm in_row_mul B=%d T=%d h=%d" % (B, T, h))


# --------------------------------------------------------------------------------------------------------------------------------
# LayerNorm-prep (pre-LN + fold entry)
# --------------------------------------------------------------------------------------------------------------------------------
def run_rows(L, op, in0, in1, idx, n, out0, out1=None):
    n = list(n) + [0] * (5 - len(n))
    rc = L.clip_amd_test_rows(op, _vp(in0), _vp(in1), _i32p(idx), n[0], n[1], n[2], n[3], n[4], _vp(out0), _vp(out1))
    assert rc == 0, "clip_amd_test_rows op %d rc=%d" % (op, rc)


@pytest.mark.parametrize("T", [0, 1, 5, 50])
@pytest.mark.parametrize("with_w", [1, 0])
@pytest.mark.parametrize("h", [64, 768, 1024, 1344])
def test_layernorm_prep(L, h, with_w, T):
    """The fused entry against the two launches forward.cpp falls back to: out32 must equal launch_cls_rows + launch_layernorm on the same data
    BITWISE (the same arithmetic per row), and that two-launch result is itself held to the oracle's LayerNorm of x with numpy's class rows
    (atol 2e-5, rtol 1e-5).  T > 0: rows r % T == 0 are class_embd + pos0 built in registers; x holds NaN there, which must never be read.
    w == NULL: no LayerNorm, y = x, and out32 is not written at all.  xg, mu and the statistics are those of y: check_fold.  Each case runs
    centred and uncentred, in place (out32 aliases x) and out of place."""
    rng = np.random.default_rng(h * 131 + T * 7 + with_w)
    rows = {0: 37, 1: 7, 5: 25, 50: 150}[T]
    assert rows % 4 != 0
    ldx, ld32, ldxg = h + 4, h + 8, h + 4
    x = rows_data(rng, rows, h, ldx)
    w, b = ln_params(rng, h) if with_w else (None, None)
    g = (1 + rng.standard_normal(h) * 0.1).astype(np.float32)
    cls = pos0 = None
    full = x[:, :h].copy()                       # the rows the kernel works on, by numpy
    if T:
        cls, pos0 = (rng.standard_normal(h) * 0.5).astype(np.float32), (rng.standard_normal(h) * 0.5).astype(np.float32)
        x[::T, :h] = np.nan
        full[::T] = cls + pos0
        two = np.ascontiguousarray(x[:, :h])       # two-launch form, first launch: class rows into x
        run_rows(L, 0, cls, pos0, None, (rows // T, T, h), two)
        assert_bits_equal(two, full, "cls_rows")
    if with_w:
        _, y = run_ln(L, full, w, b, rows, h, want16=False)    # two-launch form, second launch
        y = np.ascontiguousarray(y[:, :h])
        np.testing.assert_allclose(y, ref.layer_norm(full, w, b, EPS), atol=2e-5, rtol=1e-5)
    else:
        y = full
    for centred in (0, 1):
        for in_place in (0, 1):
            what = "layernorm_prep h=%d w=%d T=%d centred=%d in_place=%d" % (h, with_w, T, centred, in_place)
            ld_o = ldx if in_place else ld32
            out, xg, stats, mu = np.empty((rows, ld_o), np.float32), np.empty((rows, ldxg), np.uint16), np.empty((rows, 2), np.float32), np.empty(rows, np.float32)
            rc = L.clip_amd_test_layernorm_prep(_fp(x), ldx, _fp(w), _fp(b), EPS, rows, h, _fp(g), centred, _fp(cls), _fp(pos0), T, in_place,
                                                _fp(out), ld_o, _u16p(xg), ldxg, _fp(stats), _fp(mu))
            assert rc == 0, "clip_amd_test_layernorm_prep rc=%d" % rc
            if with_w:
                assert_bits_equal(out[:, :h], y, what + " out32 against cls_rows + layernorm")
                assert_bits_equal(bits32(out[:, h:]), bits32(x[:, h:]) if in_place else np.full((rows, ld_o - h), POISON32, np.uint32), what + " out32 padding")
            elif in_place:
                assert_bits_equal(out, x, what + " x (no LayerNorm: not written)")
            else:
                assert_poison(out, what + " out32 (no LayerNorm: not written)")
            check_fold(y, g, h, centred, xg, stats, mu, what)


# --------------------------------------------------------------------------------------------------------------------------------
# small kernels
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,h", [(3, 5, 320), (5, 1, 64), (7, 50, 1344)])
def test_cls_rows(L, B, T, h):
    """x[b T] = f32(class_embd + pos[0]): one rounding, bitwise; every other row keeps its bits.  B h is no multiple of the workgroup's 256."""
    assert (B * h) % 256 != 0
    rng = np.random.default_rng(B * T + h)
    cls, pos = rng.standard_normal(h).astype(np.float32), rng.standard_normal((T + 1, h)).astype(np.float32)
    x0 = rows_data(rng, B * T, h)
    want = x0.copy()
    want[::T] = cls + pos[0]
    x = x0.copy()
    run_rows(L, 0, cls, pos, None, (B, T, h), x)
    assert_bits_equal(x, want, "cls_rows B=%d T=%d h=%d" % (B, T, h))


@pytest.mark.parametrize("with_a", [1, 0])
@pytest.mark.parametrize("h", [64, 1280, 2048])
def test_gather_rows(L, h, with_a):
    """xp[r] = x[src(r)], ap[r] = a[src(r)], src(r) = in_rows[r] or r in_row_mul: copies, bitwise; a == NULL: ap is not written."""
    rng = np.random.default_rng(h + with_a)
    n_src, rows = 23, 11
    x = rows_data(rng, n_src, h)
    a = rng.integers(0, 65536, size=(n_src, h)).astype(np.uint16) if with_a else None
    in_rows = rng.integers(0, n_src, size=rows).astype(np.int32)
    in_rows[:3] = (n_src - 1, 0, n_src - 1)
    for idx, mul, src in ((in_rows, 1, in_rows), (None, 2, np.arange(rows) * 2), (None, 1, np.arange(rows))):
        xp, ap = np.empty((rows, h), np.float32), np.empty((rows, h), np.uint16)
        run_rows(L, 1, x, a, idx, (rows, mul, h, n_src), xp, ap)
        what = "gather_rows h=%d %s" % (h, "in_rows" if idx is not None else "in_row_mul=%d" % mul)
        assert_bits_equal(xp, x[src], what + " xp")
        if with_a:
            assert_bits_equal(ap, a[src], what + " ap")
        else:
            assert_poison(ap, what + " ap without a")


@pytest.mark.parametrize("n", [4, 64, 500, 512, 768, 1024])
@pytest.mark.parametrize("rows", [1, 6])
def test_l2norm(L, rows, n):
    """normalize = 0: out = v 1.0f, a bitwise copy.  normalize = 1: out = v (1 / sqrt(sum v^2)) against float64, in units of |v| / ||v||: a term of
    the sum of squares carries its own rounding, at most ceil(n / 64) lane additions and 6 shuffle levels, c = ceil(n / 64) + 7 roundings, all
    terms positive, so the sum is off by at most gamma(c) relatively and its square root by half of that; then come the square root, the
    division (both correctly rounded: the HIP default for f32) and the final product, one rounding each:
        |out - v / ||v||| <= gamma(c / 2 + 3) |v| / ||v||."""
    rng = np.random.default_rng(rows * 2000 + n)
    v = (rng.standard_normal((rows, n)) * rng.uniform(0.01, 30, size=(rows, 1))).astype(np.float32)
    out = np.empty_like(v)
    run_rows(L, 2, v, None, None, (rows, n, 0), out)
    assert_bits_equal(out, v, "l2norm normalize=0")
    run_rows(L, 2, v, None, None, (rows, n, 1), out)
    v64 = v.astype(np.float64)
    want = v64 / np.sqrt((v64 ** 2).sum(1, keepdims=True))
    bound = gamma((-(-n // 64) + 7) / 2 + 3) * np.abs(want)
    err = np.abs(out - want)
    print("l2norm rows=%d n=%d: max error / bound %.3f" % (rows, n, (err / bound).max()))
    assert (err <= bound).all(), "l2norm off by %g of its bound" % (err / bound).max()


@pytest.mark.parametrize("h", [64, 768, 2048])
def test_row_stats(L, h):
    """Slot 0 of the [row][128 slots] layout := (sum x, sum x^2), the other 127 slots are not written.  Against float64 sums: an element passes
    through 2 additions inside its float4, at most ceil(h / 256) accumulations and 6 shuffle levels, and its square carries one more rounding:
        |s1 - S1| <= gamma(ceil(h / 256) + 8) sum|x|,     |s2 - S2| <= gamma(ceil(h / 256) + 9) sum x^2."""
    rng = np.random.default_rng(h)
    rows, ldx = 7, h + 4
    x = rows_data(rng, rows, h, ldx)
    st = np.empty((rows, 128, 2), np.float32)
    run_rows(L, 3, x, None, None, (rows, h, ldx), st)
    x64 = x[:, :h].astype(np.float64)
    ni = -(-h // 256)
    e1, b1 = np.abs(st[:, 0, 0] - x64.sum(1)), gamma(ni + 8) * np.abs(x64).sum(1)
    e2, b2 = np.abs(st[:, 0, 1] - (x64 ** 2).sum(1)), gamma(ni + 9) * (x64 ** 2).sum(1)
    print("row_stats h=%d: max error / bound %.3f (sum) %.3f (squares)" % (h, (e1 / b1).max(), (e2 / b2).max()))
    assert (e1 <= b1).all() and (e2 <= b2).all(), "row_stats off by %g / %g of its bounds" % ((e1 / b1).max(), (e2 / b2).max())
    assert_poison(st[:, 1:], "row_stats slots 1..127")


def test_f32_to_f16(L):
    """dst[r][c] = fp16(src[r][c]) for c < cols (round to nearest even, ties and overflow to infinity included: numpy's astype), +0 for
    cols <= c < cols_pad, not written for cols_pad <= c < ldd.  The source's padding holds NaN."""
    rng = np.random.default_rng(5)
    rows, cols, cols_pad, lds, ldd = 5, 70, 96, 76, 104
    src = nan32((rows, lds))
    src[:, :cols] = tie_pixels(rng, (rows, cols))
    src[0, :6] = (65504.0, 65519.99, 65520.0, -65520.0, 1e-8, -0.0)
    dst = np.empty((rows, ldd), np.uint16)
    run_rows(L, 4, src, None, None, (rows, cols, cols_pad, lds, ldd), dst)
    with np.errstate(over="ignore"):
        want = src[:, :cols].astype(np.float16)
    assert_bits_equal(dst[:, :cols], bits16(want), "f32_to_f16")
    assert (dst[:, cols:cols_pad] == 0).all(), "cols..cols_pad must be +0"
    assert_poison(dst[:, cols_pad:], "f32_to_f16 ldd padding")


def test_f16_to_f32(L):
    """Widening is exact: every finite fp16 (subnormals included) and both infinities, bitwise; the ldd padding is not written."""
    rng = np.random.default_rng(6)
    rows, cols, lds, ldd = 13, 1000, 1024, 1008
    src = rng.integers(0, 65536, size=(rows, lds)).astype(np.uint16)
    src[0, :6] = (0x0000, 0x8000, 0x0001, 0x83ff, 0x7c00, 0xfc00)
    is_nan = ((src & 0x7c00) == 0x7c00) & ((src & 0x03ff) != 0)
    src[is_nan] &= 0xfc00                                    # NaN payloads -> infinity of the same sign
    dst = np.empty((rows, ldd), np.float32)
    run_rows(L, 5, src, None, None, (rows, cols, 0, lds, ldd), dst)
    assert_bits_equal(dst[:, :cols], np.ascontiguousarray(src[:, :cols]).view(np.float16).astype(np.float32), "f16_to_f32")
    assert_poison(dst[:, cols:], "f16_to_f32 ldd padding")
