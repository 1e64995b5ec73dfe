"""clip_amd_test_gemm_f32 checks its arguments on the host before it looks for a device: what the kernel's 4-column epilogues and the patch
scatter cannot take is refused with -3 whether or not a GPU is there (no device would be -1), nothing is launched, and y comes back
untouched.  Needs the library, no device.  The kernel itself is tested in test_gpu_gemm_f32.py."""
import numpy as np

import gemm_f32_common as gc

M, N, K = 8, 64, 64
NP, T = 4, 5


def _refused(L, what, **kw):
    rng = np.random.default_rng(5)
    W = rng.standard_normal((N, K)).astype(np.float32)
    X = rng.standard_normal((M, K)).astype(np.float32)
    rc, y = gc.call_gemm_f32(L, W, X, **kw)
    assert rc == -3, (what, rc)
    assert np.all(y.view(np.uint32) == gc.SENTINEL_BITS), (what, "y was written")


def test_hook_refuses_what_the_kernel_cannot_take(clip_lib):
    L = clip_lib.lib()
    pos = np.zeros((T, N), np.float32)
    resid = np.zeros((M, N), np.float32)
    patch = dict(epi=5, Np=NP, T=T, pos=pos, act_f32=0)
    _refused(L, "N % 4", N=N - 2)
    _refused(L, "N % 4, residual epilogue", N=N - 1, epi=4, resid=resid)
    _refused(L, "qcols % 4", epi=1, qcols=6, qscale=0.5)
    _refused(L, "qcols > N", epi=1, qcols=N + 4, qscale=0.5)
    _refused(L, "qcols < 0", epi=1, qcols=-4, qscale=0.5)
    _refused(L, "patch epilogue with f32 activations", **dict(patch, act_f32=1))
    _refused(L, "Np = 0", **dict(patch, Np=0))
    _refused(L, "Np < 0", **dict(patch, Np=-NP))
    _refused(L, "T < Np + 1", **dict(patch, T=NP))
    _refused(L, "M % Np", **dict(patch, Np=3, T=4))
    _refused(L, "patch epilogue without pos", **dict(patch, pos=None))
    _refused(L, "residual epilogue without resid", epi=4)
    _refused(L, "epilogue 6", epi=6)
    _refused(L, "epilogue -1", epi=-1)
    _refused(L, "act_f32 = 2", act_f32=2)
    _refused(L, "guard_rows < 0", guard=-1)
