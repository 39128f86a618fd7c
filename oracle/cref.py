"""ctypes binding of oracle/mix_ref.c (TEST INFRASTRUCTURE ONLY; see oracle/__init__.py)."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "_build", "libmixref.so")
_lib = None


def build():
    import subprocess
    subprocess.run(["make", "-s", "-C", _HERE], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            build()
        L = ctypes.CDLL(_LIB)
        P = ctypes.c_void_p
        i32, i64, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        L.ref_mix_round.argtypes = [P, i64, P, i64, f32, P, i64, i32, i64, P, P, P, P, i64]
        L.ref_mix_round.restype = None
        L.ref_column_mean.argtypes = [P, i64, i32, i64, P]
        L.ref_column_mean.restype = None
        L.ref_deviation_sq.argtypes = [P, i64, i32, i64, P, P]
        L.ref_deviation_sq.restype = None
        L.ref_sgd_step.argtypes = [P, i64, P, i64, P, i64, P, i64, i32, i64, f32, f32, f32, f32,
                                   i32, i32]
        L.ref_sgd_step.restype = None
        L.ref_bgemm.argtypes = [i32, i32, i32, i32, P, i64, i64, i32, P, i64, i64, i32,
                                P, i64, i64, i32, P, i64, P, i64, i64, P, P, i64]
        L.ref_bgemm.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def mix_round(X, rowptr, cols, w, G=None, lr=0.0, block=4096):
    """C restatement of Mixer._mix_params_once (+ optional fused ``x - lr*g``)."""
    X = np.ascontiguousarray(X, np.float32)
    n, p = X.shape
    out = np.empty_like(X)
    rp = np.ascontiguousarray(rowptr, np.int64)
    cl = np.ascontiguousarray(cols, np.int64)
    ww = np.ascontiguousarray(w, np.float64)
    scratch = None
    if G is not None:
        G = np.ascontiguousarray(G, np.float32)
        scratch = np.empty((n, block), np.float32)
    lib().ref_mix_round(_p(X), p, _p(G), p, float(lr), _p(out), p, n, p, _p(rp), _p(cl), _p(ww),
                        _p(scratch), block)
    return out


def column_mean(X):
    X = np.ascontiguousarray(X, np.float32)
    m = np.empty(X.shape[1], np.float32)
    lib().ref_column_mean(_p(X), X.shape[1], X.shape[0], X.shape[1], _p(m))
    return m


def deviation_sq(X, mean=None):
    X = np.ascontiguousarray(X, np.float32)
    if mean is None:
        mean = column_mean(X)
    d = np.empty(X.shape[0], np.float64)
    lib().ref_deviation_sq(_p(X), X.shape[1], X.shape[0], X.shape[1], _p(mean), _p(d))
    return d


def bgemm(batch, M, N, K, A, lda, sA, ta, B, ldb, sB, tb, C, ldc, sC, epi=0, bias=None, s_bias=0,
          H=None, ldh=0, sH=0, C2=None, rowsum=None, s_rowsum=0):
    """dl_bgemm as a k-ordered fp32 fma chain (ref_bgemm in mix_ref.c; arguments as
    dl_bgemm_args).  A, B, bias, H and the outputs C, C2 (epi 6: the second DTANH candidate),
    rowsum are flat contiguous fp32 arrays; the outputs are written in place, logical elements
    only.  For epi 3, 4 and 8 C receives the pre-activation z."""
    def span(rows, width, ld, stride):   # one past the last element addressed
        return (batch - 1) * stride + (rows - 1) * ld + width
    need = [(A, span(K if ta else M, M if ta else K, lda, sA)),
            (B, span(N if tb else K, K if tb else N, ldb, sB)), (C, span(M, N, ldc, sC))]
    if bias is not None:
        need.append((bias, span(1, N, 0, s_bias)))
    if 5 <= epi <= 7:
        need.append((H, span(M, N, ldh, sH)))
    if epi == 6:
        need.append((C2, span(M, N, ldc, sC)))
    if rowsum is not None:
        need.append((rowsum, span(1, M, 0, s_rowsum)))
    for arr, n in need:
        if arr is None or arr.dtype != np.float32 or not arr.flags.c_contiguous or arr.size < n:
            raise ValueError("bgemm: operands must be contiguous fp32 arrays covering their span")
    if min(batch, M, N, K, lda, ldb, ldc, sA, sB, sC, s_bias, s_rowsum) < 0 or ldh < 0 or sH < 0:
        raise ValueError("bgemm: negative size or stride")
    lib().ref_bgemm(batch, M, N, K, _p(A), lda, sA, int(ta), _p(B), ldb, sB, int(tb), _p(C), ldc,
                    sC, int(epi), _p(bias), s_bias, _p(H), ldh, sH, _p(C2), _p(rowsum), s_rowsum)


def sgd_step(X, G, buf=None, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0,
             nesterov=False, first=False):
    """C restatement of torch.optim.SGD.step over agent rows.  Returns the stepped X; ``buf`` is
    updated in place (a new zero buffer when None and momentum != 0)."""
    X = np.ascontiguousarray(X, np.float32)
    G = np.ascontiguousarray(G, np.float32)
    n, p = X.shape
    if momentum != 0.0 and buf is None:
        buf = np.zeros_like(X)
    out = np.empty_like(X)
    lib().ref_sgd_step(_p(X), p, _p(G), p, _p(buf), p, _p(out), p, n, p, float(lr),
                       float(momentum), float(dampening), float(weight_decay), int(nesterov),
                       int(first))
    return out
