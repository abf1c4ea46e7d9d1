"""The fp8 quantisation entry points (quant_fp8.hip) without a GPU: the six symbols are declared, exported and bound, and
every argument-error and not-supported status is returned before any device work (fake pointers, never dereferenced)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [base + sfx for base in ("sm_quantize_rows_fp8_", "sm_quantize_compress24_fp8_", "sm_quantize_transpose_fp8_") for sfx in ("f16", "bf16")]
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
E4M3, E5M2 = 0, 1
SFX = ["f16", "bf16"]


def test_symbols_exported_declared_and_bound(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    for fn in ("quantize_rows_fp8", "quantize_compress24_fp8", "quantize_transpose_fp8"):
        assert callable(getattr(pkg, fn))


def _rows(pkg, sfx, A=P, rows=8, k=64, lda=None, Q=P, ldq=None, rs=P, fmt=E4M3):
    fn = getattr(pkg.lib(), "sm_quantize_rows_fp8_" + sfx)
    return fn(A, rows, k, k if lda is None else lda, Q, k if ldq is None else ldq, rs, fmt, None)


def _comp(pkg, sfx, A=P, rows=8, k=64, lda=None, blob=P, rs=P, fmt=E4M3):
    fn = getattr(pkg.lib(), "sm_quantize_compress24_fp8_" + sfx)
    return fn(A, rows, k, k if lda is None else lda, blob, rs, fmt, None)


def _tr(pkg, sfx, B=P, k=64, n=8, ldb=None, inv=1.0, Bt=P, fmt=E4M3):
    fn = getattr(pkg.lib(), "sm_quantize_transpose_fp8_" + sfx)
    return fn(B, k, n, n if ldb is None else ldb, inv, Bt, fmt, None)


@pytest.mark.parametrize("sfx", SFX)
def test_quantize_rows_statuses_without_a_device(pkg, sfx):
    for kw in (dict(A=None), dict(Q=None), dict(rs=None), dict(fmt=2), dict(fmt=-1), dict(lda=56), dict(ldq=63)):
        assert _rows(pkg, sfx, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    for kw in (dict(A=ODD), dict(lda=68), dict(k=100, lda=100), dict(rows=BIG), dict(k=BIG, lda=BIG, ldq=BIG), dict(lda=BIG), dict(ldq=BIG)):
        assert _rows(pkg, sfx, **kw) == NOT_SUPPORTED, kw
    # the dense form takes any k (rows of A still 16-byte aligned) and any ldq; nothing to do: success, pointers untouched
    for fmt in (E4M3, E5M2):
        assert _rows(pkg, sfx, rows=0, fmt=fmt) == 0
        assert _rows(pkg, sfx, k=0, fmt=fmt) == 0
        assert _rows(pkg, sfx, rows=0, k=100, lda=104, ldq=101, Q=ODD, fmt=fmt) == 0


@pytest.mark.parametrize("sfx", SFX)
def test_quantize_compress_statuses_without_a_device(pkg, sfx):
    for kw in (dict(A=None), dict(blob=None), dict(rs=None), dict(fmt=2), dict(fmt=-1), dict(lda=56), dict(blob=ODD)):
        assert _comp(pkg, sfx, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    for kw in (dict(A=ODD), dict(lda=68), dict(k=96), dict(k=100, lda=104), dict(rows=BIG), dict(k=BIG, lda=BIG), dict(lda=BIG)):
        assert _comp(pkg, sfx, **kw) == NOT_SUPPORTED, kw
    for fmt in (E4M3, E5M2):
        assert _comp(pkg, sfx, rows=0, fmt=fmt) == 0
        assert _comp(pkg, sfx, k=0, fmt=fmt) == 0


@pytest.mark.parametrize("sfx", SFX)
def test_quantize_transpose_statuses_without_a_device(pkg, sfx):
    for kw in (dict(B=None), dict(Bt=None), dict(fmt=2), dict(fmt=-1), dict(ldb=7)):
        assert _tr(pkg, sfx, **kw) == INVALID, kw
        assert b"invalid" in pkg.lib().sm_last_error()
    for kw in (dict(k=BIG), dict(n=BIG, ldb=BIG), dict(ldb=BIG)):
        assert _tr(pkg, sfx, **kw) == NOT_SUPPORTED, kw
    assert _tr(pkg, sfx, k=0) == 0
    assert _tr(pkg, sfx, n=0) == 0


def test_python_wrappers_refuse_wrong_dtypes(pkg):
    torch = pytest.importorskip("torch")
    A16 = torch.zeros(8 * 64, dtype=torch.float16)
    q8 = torch.zeros(8 * 64, dtype=torch.uint8)
    rs = torch.zeros(8, dtype=torch.float32)
    blob = torch.zeros(1024, dtype=torch.uint8)
    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    # every refusal below is about a dtype and comes before any pointer is taken
    for bad_a in (A16.float(), A16.double(), q8, q8.view(e4)):
        with pytest.raises(pkg.SparsifymeError, match="float16 or bfloat16"):
            pkg.quantize_rows_fp8(bad_a, q8.view(e4), rs, 8, 64)
        with pytest.raises(pkg.SparsifymeError, match="float16 or bfloat16"):
            pkg.quantize_compress24_fp8(bad_a, blob, rs, 8, 64, e4)
        with pytest.raises(pkg.SparsifymeError, match="float16 or bfloat16"):
            pkg.quantize_transpose_fp8(bad_a, q8.view(e5), 64, 8, 1.0)
    for bad_q in (q8, q8.view(torch.int8), q8.view(torch.float8_e4m3fnuz), q8.view(torch.float8_e5m2fnuz)):
        with pytest.raises(pkg.SparsifymeError, match="float8_e4m3fn or torch.float8_e5m2"):
            pkg.quantize_rows_fp8(A16, bad_q, rs, 8, 64)
        with pytest.raises(pkg.SparsifymeError, match="float8_e4m3fn or torch.float8_e5m2"):
            pkg.quantize_compress24_fp8(A16, blob, rs, 8, 64, bad_q.dtype)
        with pytest.raises(pkg.SparsifymeError, match="float8_e4m3fn or torch.float8_e5m2"):
            pkg.quantize_transpose_fp8(A16, bad_q, 64, 8, 1.0)
    for bad_rs in (rs.double(), rs.half(), rs.to(torch.int32)):
        with pytest.raises(pkg.SparsifymeError, match="row_scale is float32"):
            pkg.quantize_rows_fp8(A16.bfloat16(), q8.view(e5), bad_rs, 8, 64)
        with pytest.raises(pkg.SparsifymeError, match="row_scale is float32"):
            pkg.quantize_compress24_fp8(A16, blob, bad_rs, 8, 64, e5)
