"""Shared by test_gpu_gemm_f32.py and test_gemm_f32_hook_cpu.py: the call of clip_amd_test_gemm_f32 (include/clip_amd.h)."""
import ctypes as C

import numpy as np

SENTINEL = 777.0          # exact in fp16: the fill survives the fp16 round trip of the hook's act_f32 = 0 form bit for bit
SENTINEL_BITS = np.float32(SENTINEL).view(np.uint32)
GUARD_ROWS = 2


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def call_gemm_f32(L, W, X, bias=None, resid=None, epi=0, qcols=0, qscale=1.0, Np=0, T=0, pos=None, act_f32=1, guard=GUARD_ROWS, N=None):
    """-> (rc, y): y [rows + guard][N] f32 as the hook left it, SENTINEL wherever nothing was written; rows = M, for epilogue 5 (M / Np) T.
    N overrides the weight's row count in the call (the refusals of the CPU test: the buffers keep their real size)."""
    W, X, bias, resid, pos = _f32(W), _f32(X), _f32(bias), _f32(resid), _f32(pos)
    K, M = W.shape[1], X.shape[0]
    N = W.shape[0] if N is None else N
    rows = (M // Np) * T if epi == 5 and Np > 0 and T > 0 else M
    y = np.full((rows + max(guard, 0), max(N, W.shape[0])), SENTINEL, dtype=np.float32)
    rc = L.clip_amd_test_gemm_f32(W.ctypes.data_as(C.c_void_p), N, K, _fp(X), M, _fp(bias), _fp(resid), epi, qcols, qscale, Np, T, _fp(pos),
                                  act_f32, guard, _fp(y))
    return rc, y


def run_gemm_f32(L, W, X, what="", **kw):
    """The hook on a valid case: rc == 0, the guard rows still hold the sentinel bit for bit; -> y [rows][N]."""
    guard = kw.get("guard", GUARD_ROWS)
    rc, y = call_gemm_f32(L, W, X, **kw)
    assert rc == 0, (what, "clip_amd_test_gemm_f32 rc=%d" % rc)
    rows = y.shape[0] - guard
    tail = y[rows:]
    assert np.all(tail.view(np.uint32) == SENTINEL_BITS), (what, "rows past the last one were written", int((tail.view(np.uint32) != SENTINEL_BITS).sum()))
    return y[:rows]
