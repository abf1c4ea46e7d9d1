"""The OCP fp8 2:4 entry points without a GPU: the six symbols are declared and exported, and every argument-error and
not-supported status is returned before any device work (fake pointers, never dereferenced)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sm_prune24_fp8", "sm_prune24_check_fp8", "sm_compress24_fp8", "sm_decompress24_fp8", "sm_spmma_fp8", "sm_spmma_fused_fp8"]
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
E4M3, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2


def test_symbols_exported_and_declared(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    for macro, value in [("SM_FP8_E4M3", 0), ("SM_FP8_E5M2", 1), ("SM_OUT_F32", 0), ("SM_OUT_F16", 1), ("SM_OUT_BF16", 2)]:
        assert f"#define {macro} {value}" in header


def _spmma(pkg, blob=P, B=P, C=P, m=64, n=32, k=128, batch=2, strideB=0, strideC=None, fa=E4M3, fb=E4M3, ot=F32):
    strideC = m * n if strideC is None else strideC
    return pkg.lib().sm_spmma_fp8(blob, B, C, m, n, k, batch, strideB, strideC, fa, fb, ot, 1.0, 0.0, None, None)


def _fused(pkg, A=P, B=P, C=P, m=64, n=32, k=128, lda=None, batch=2, strideA=None, strideB=0, strideC=None, fa=E4M3, fb=E4M3, ot=F32):
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    return pkg.lib().sm_spmma_fused_fp8(A, B, C, m, n, k, lda, batch, strideA, strideB, strideC, fa, fb, ot, 1.0, 0.0, None, None)


@pytest.mark.parametrize("call", [_spmma, _fused])
def test_matmul_statuses_without_a_device(pkg, call):
    first = "blob" if call is _spmma else "A"
    for kw in ({first: None}, dict(B=None), dict(C=None), dict(fa=2), dict(fb=-1), dict(ot=3), dict(ot=-1)):
        assert call(pkg, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    for kw in (dict(k=100), dict(k=96), dict(m=63), dict(B=ODD), dict(strideB=8), dict(m=BIG, strideC=0), dict(n=BIG, strideC=0),
               dict(k=BIG)):
        assert call(pkg, **kw) == NOT_SUPPORTED, kw
    # nothing to do: success without touching the (fake) pointers
    assert call(pkg, m=0) == 0
    assert call(pkg, n=0) == 0
    assert call(pkg, batch=0) == 0


def test_blob_and_fused_a_alignment(pkg):
    assert _spmma(pkg, blob=ODD) == INVALID          # the blob is 16-byte aligned by contract
    assert _fused(pkg, A=ODD) == NOT_SUPPORTED       # unaligned rows of A: use compress + spmma
    assert _fused(pkg, k=128, lda=136) == NOT_SUPPORTED
    assert _fused(pkg, k=128, lda=64) == INVALID     # lda < k
    assert _fused(pkg, lda=BIG) == NOT_SUPPORTED


def test_streaming_statuses_without_a_device(pkg):
    L = pkg.lib()
    for args in ((None, P, 8, 8, 8, 1, E4M3), (P, None, 8, 8, 8, 1, E4M3), (P, P, 8, 8, 4, 1, E4M3), (P, P, 8, 8, 8, 2, E4M3),
                 (P, P, 8, 8, 8, 1, 2), (P, P, 8, 8, 8, 0, -1)):
        assert L.sm_prune24_fp8(*args, None) == INVALID, args
    for fmt in (E4M3, E5M2):
        for alg in (0, 1):
            assert L.sm_prune24_fp8(P, P, 0, 8, 8, alg, fmt, None) == 0
            assert L.sm_prune24_fp8(P, P, 8, 0, 8, alg, fmt, None) == 0
    assert L.sm_prune24_check_fp8(None, 8, 8, 8, P, None) == INVALID
    assert L.sm_prune24_check_fp8(P, 8, 8, 8, None, None) == INVALID
    assert L.sm_prune24_check_fp8(P, 8, 8, 4, P, None) == INVALID
    for args in ((None, 8, 64, 64, 1, 512, P, E4M3), (P, 8, 64, 64, 1, 512, None, E4M3), (P, 8, 64, 32, 1, 512, P, E4M3),
                 (P, 8, 64, 64, 1, 512, ODD, E4M3), (P, 8, 64, 64, 1, 512, P, 5)):
        assert L.sm_compress24_fp8(*args, None) == INVALID, args
    assert L.sm_compress24_fp8(P, 0, 64, 64, 1, 0, P, E5M2, None) == 0
    assert L.sm_compress24_fp8(P, 8, 64, 64, 0, 512, P, E4M3, None) == 0
    assert L.sm_decompress24_fp8(None, 8, 64, 64, 1, 512, P, None) == INVALID
    assert L.sm_decompress24_fp8(P, 8, 64, 64, 1, 512, None, None) == INVALID
    assert L.sm_decompress24_fp8(P, 0, 64, 64, 1, 0, P, None) == 0


def test_python_wrappers_refuse_wrong_dtypes(pkg):
    torch = pytest.importorskip("torch")
    with pytest.raises(pkg.SparsifymeError):
        pkg.fp8_format(torch.int8)
    with pytest.raises(pkg.SparsifymeError):
        pkg.fp8_format(torch.float8_e4m3fnuz)
    assert pkg.fp8_format(torch.float8_e4m3fn) == E4M3 and pkg.fp8_format(torch.float8_e5m2) == E5M2
    for dt in (torch.int32, torch.float64, torch.int8):
        with pytest.raises(pkg.SparsifymeError):
            pkg._fp8_out_type(torch.empty(1, dtype=dt))
