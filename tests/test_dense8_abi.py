"""The dense fp8 / int8 GEMM entry points without a GPU: the three symbols are declared, bound and exported, and every
argument-error and not-supported status is returned before any device work (fake pointers, never dereferenced)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sm_gemm_rowmajor_fp8", "sm_gemm_rowmajor_i8", "sm_gemm_rowmajor_i8_q"]
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
E4M3, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2


def test_symbols_declared_bound_and_exported(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    for name in ("gemm_rowmajor_fp8", "gemm_rowmajor_i8", "gemm_rowmajor_i8_q"):
        assert callable(getattr(pkg, name))


def _fp8(pkg, A=P, B=P, C=P, m=64, n=32, k=128, lda=None, batch=2, strideA=None, strideB=0, strideC=None, fa=E4M3, fb=E4M3, ot=F32):
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    return pkg.lib().sm_gemm_rowmajor_fp8(A, B, C, m, n, k, lda, batch, strideA, strideB, strideC, fa, fb, ot, 1.0, 0.0, None, None)


def _i8(pkg, A=P, B=P, C=P, m=64, n=32, k=128, lda=None, batch=2, strideA=None, strideB=0, strideC=None):
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    return pkg.lib().sm_gemm_rowmajor_i8(A, B, C, m, n, k, lda, batch, strideA, strideB, strideC, 0, None)


def _i8q(pkg, A=P, B=P, C=P, m=64, n=32, k=128, lda=None, batch=2, strideA=None, strideB=0, strideC=None):
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    return pkg.lib().sm_gemm_rowmajor_i8_q(A, B, C, m, n, k, lda, batch, strideA, strideB, strideC, 0.5, None)


CALLS = [_fp8, _i8, _i8q]


@pytest.mark.parametrize("call", CALLS)
def test_statuses_without_a_device(pkg, call):
    for kw in (dict(A=None), dict(B=None), dict(C=None), dict(k=128, lda=64)):
        assert call(pkg, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    for kw in (dict(k=100), dict(k=96), dict(k=32), dict(A=ODD), dict(B=ODD), dict(k=128, lda=136), dict(strideA=8),
               dict(strideB=8), dict(m=BIG, strideC=0), dict(n=BIG, strideC=0), dict(k=BIG), dict(lda=BIG), dict(m=BIG // 2, batch=2)):
        assert call(pkg, **kw) == NOT_SUPPORTED, kw
    # nothing to do: success without touching the (fake) pointers
    assert call(pkg, m=0) == 0
    assert call(pkg, n=0) == 0
    assert call(pkg, batch=0) == 0


def test_fp8_format_and_output_statuses(pkg):
    for kw in (dict(fa=2), dict(fa=-1), dict(fb=2), dict(fb=-1), dict(ot=3), dict(ot=-1)):
        assert _fp8(pkg, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    # a bad format is an argument error even where there is nothing to compute
    assert _fp8(pkg, m=0, fa=7) == INVALID


def test_python_wrappers_refuse_wrong_dtypes(pkg):
    torch = pytest.importorskip("torch")
    a8 = torch.empty(1, dtype=torch.float8_e4m3fn)
    with pytest.raises(pkg.SparsifymeError):
        pkg.gemm_rowmajor_fp8(torch.empty(1, dtype=torch.int8), a8, torch.empty(1), 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError):
        pkg.gemm_rowmajor_fp8(a8, a8, torch.empty(1, dtype=torch.int32), 1, 1, 64)
    i8 = torch.empty(1, dtype=torch.int8)
    with pytest.raises(pkg.SparsifymeError):
        pkg.gemm_rowmajor_i8(i8, i8, torch.empty(1, dtype=torch.int8), 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError):
        pkg.gemm_rowmajor_i8_q(i8, i8, torch.empty(1, dtype=torch.int32), 1, 1, 64, 1.0)
