"""GPU tier of the hubness column of the exact index (bias_fold_kernel of k_bias.hip, clip_amd_index_hubness): bit for bit against the
pre-existing cross-index calls it is built on (bank.search_index / bank.softmax_index of the gallery's rows) folded in numpy f32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, S = 10, 100.0


@pytest.fixture(scope="module")
def clip(clip_lib, fixture_cache):
    from oracle import fixtures
    if clip_lib.device_count() < 1:
        pytest.fail("no HIP device")
    m = clip_lib.Clip(fixtures.cached_model(fixture_cache, "tiny", "f32"), verbosity=0, device=0)
    yield m
    m.close()


def reference(bank, ix, mode):
    if mode == "softmax":
        return (bank.softmax_index(ix, 1, S)[3] / np.float32(S)).astype(np.float32)
    d, i = bank.search_index(ix, K)
    total, count = np.zeros(len(ix), dtype=np.float32), np.zeros(len(ix), dtype=np.float32)
    for j in range(K):                                      # present slots in ascending slot order, f32
        total = np.where(i[:, j] >= 0, total + d[:, j], total).astype(np.float32)
        count += i[:, j] >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count > 0, total * (np.float32(-0.5) / count), np.float32(0)).astype(np.float32)


@pytest.mark.parametrize("mode", ["csls", "softmax"])
@pytest.mark.parametrize("dtype, n, n_bank", [("f16", 1030, 5), ("i8", 1030, 300), ("f32", 1030, 300), ("f16", 65537, 300), ("i8", 65537, 5)])
def test_hubness_column(clip, clip_lib, mode, dtype, n, n_bank):
    dim = 36
    rng = np.random.default_rng(n + n_bank)
    ix, bank, empty = (clip_lib.Index(clip, dim, dtype) for _ in range(3))
    ix.add(rng.standard_normal((n, dim), dtype=np.float32))
    bank.add(rng.standard_normal((n_bank, dim), dtype=np.float32))
    want = reference(bank, ix, mode)                        # (before any removal: search_index takes no source with removed rows)
    got = ix.hubness(bank, mode=mode, k=K, scale=S)
    assert got.tobytes() == want.tobytes() and np.all(got != 0)
    assert not ix.hubness(empty, mode=mode, k=K, scale=S).any()
    # removed rows and rows outside allow are exactly 0, the others unchanged
    gone = rng.permutation(n)[:n // 10]
    allow = rng.random(n) < 0.7
    ix.remove(gone)
    got = ix.hubness(bank, mode=mode, k=K, scale=S, allow=allow)
    keep = allow.copy()
    keep[gone] = False
    assert got.tobytes() == np.where(keep, want, np.float32(0)).tobytes()
    for x in (ix, bank, empty):
        x.close()
