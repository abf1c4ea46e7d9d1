"""The epilogue entry points of the 16-bit 2:4 matmul (sm_spmma_{f16,bf16}_ex, sm_spmma_fused_{f16,bf16}_ex) without a GPU: the four
symbols are declared, exported and bound, every argument-error and not-supported status is returned before any device work (fake
pointers, never dereferenced), and the Python holder refuses wrong dtypes before it takes a pointer."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sm_spmma_f16_ex", "sm_spmma_bf16_ex", "sm_spmma_fused_f16_ex", "sm_spmma_fused_bf16_ex"]
INVALID, NOT_SUPPORTED = 1, 2
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
Q = ctypes.c_void_p(0x2000)
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
BIG = 1 << 31
SFX = ["f16", "bf16"]
COL, ROW = 0, 1
NONE, RELU, CLIPPED, LEAKY, HARDSWISH = 0, 1, 2, 3, 4


def test_symbols_exported_declared_and_bound(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    for word in ("sm_epilogue_t", "SM_BIAS_COL", "SM_BIAS_ROW", "SM_ACT_NONE", "SM_ACT_RELU", "SM_ACT_CLIPPED_RELU", "SM_ACT_LEAKY_RELU",
                 "SM_ACT_HARDSWISH"):
        assert word in header
    assert (pkg.BIAS_COL, pkg.BIAS_ROW) == (COL, ROW)
    assert (pkg.ACT_NONE, pkg.ACT_RELU, pkg.ACT_CLIPPED_RELU, pkg.ACT_LEAKY_RELU, pkg.ACT_HARDSWISH) == (NONE, RELU, CLIPPED, LEAKY, HARDSWISH)
    assert callable(pkg.Epilogue)


def test_struct_layout_matches_the_header(pkg):
    """sm_epilogue_t: { const float* bias; int bias_dim; int act; float act_arg; const void* R; size_t strideR; }"""
    S = pkg.EpilogueStruct
    assert [f[0] for f in S._fields_] == ["bias", "bias_dim", "act", "act_arg", "R", "strideR"]
    assert (S.bias.offset, S.bias_dim.offset, S.act.offset, S.act_arg.offset, S.R.offset, S.strideR.offset) == (0, 8, 12, 16, 24, 32)
    assert ctypes.sizeof(S) == 40


def _ep(pkg, bias=None, bias_dim=COL, act=NONE, act_arg=0.0, R=None, strideR=0):
    st = pkg.EpilogueStruct()
    st.bias, st.bias_dim, st.act, st.act_arg, st.R, st.strideR = bias, bias_dim, act, act_arg, R, strideR
    return st


def _staged(pkg, sfx, ep, blob=P, B=P, D=P, m=8, n=8, k=64, batch=1, beta=0.0):
    fn = getattr(pkg.lib(), "sm_spmma_%s_ex" % sfx)
    return fn(blob, B, D, m, n, k, batch, 0, m * n, 1.0, beta, ctypes.addressof(ep) if ep is not None else None, None)


def _fused(pkg, sfx, ep, A=P, B=P, D=P, m=8, n=8, k=64, lda=None, batch=1, beta=0.0):
    fn = getattr(pkg.lib(), "sm_spmma_fused_%s_ex" % sfx)
    lda = k if lda is None else lda
    return fn(A, B, D, m, n, k, lda, batch, m * lda, 0, m * n, 1.0, beta, ctypes.addressof(ep) if ep is not None else None, None)


BAD_EPILOGUES = [
    (dict(act=5), 0.0), (dict(act=-1), 0.0), (dict(bias_dim=2), 0.0), (dict(bias_dim=-1), 0.0),
    (dict(act=RELU), 0.5),                                   # beta != 0 and no residual operand
    (dict(bias=0x3000, R=None), 1.0),
    (dict(act=CLIPPED, act_arg=-1.0), 0.0), (dict(act=CLIPPED, act_arg=float("inf")), 0.0), (dict(act=CLIPPED, act_arg=float("nan")), 0.0),
]


@pytest.mark.parametrize("sfx", SFX)
def test_invalid_epilogues_are_refused_before_any_device_work(pkg, sfx):
    for kw, beta in BAD_EPILOGUES:
        for call in (_staged, _fused):
            assert call(pkg, sfx, _ep(pkg, **kw), beta=beta) == INVALID, (call.__name__, kw, beta)
            assert b"invalid epilogue" in pkg.lib().sm_last_error()
    # ... and before the shape is looked at: an invalid epilogue on a shape that is not taken is still INVALID
    assert _fused(pkg, sfx, _ep(pkg, act=7), n=12) == INVALID


@pytest.mark.parametrize("sfx", SFX)
def test_underlying_statuses_pass_through(pkg, sfx):
    relu = _ep(pkg, act=RELU)
    for ep in (None, _ep(pkg), relu):
        # what sm_spmma_* / sm_spmma_fused_* return today
        assert _staged(pkg, sfx, ep, blob=None) == INVALID
        assert _staged(pkg, sfx, ep, blob=ODD) == INVALID
        assert _staged(pkg, sfx, ep, D=None) == INVALID
        assert _staged(pkg, sfx, ep, m=BIG) == NOT_SUPPORTED
        assert _fused(pkg, sfx, ep, A=None) == INVALID
        assert _fused(pkg, sfx, ep, lda=32) == INVALID          # lda < k
        assert _fused(pkg, sfx, ep, n=12) == NOT_SUPPORTED      # n % 8 != 0: the staged pair
        assert _fused(pkg, sfx, ep, k=96, lda=104) == NOT_SUPPORTED   # ragged k with lda != k: not the span form's
        assert _fused(pkg, sfx, ep, A=ODD) == NOT_SUPPORTED
        assert _fused(pkg, sfx, ep, m=BIG) == NOT_SUPPORTED
        # nothing to do: success, pointers untouched
        assert _staged(pkg, sfx, ep, m=0) == 0 and _staged(pkg, sfx, ep, n=0) == 0 and _staged(pkg, sfx, ep, batch=0) == 0
        assert _fused(pkg, sfx, ep, m=0) == 0 and _fused(pkg, sfx, ep, n=0) == 0 and _fused(pkg, sfx, ep, batch=0) == 0
    # the thin form (n < 8, k <= 64) takes no epilogue
    assert _fused(pkg, sfx, relu, m=64, n=1, k=9) == NOT_SUPPORTED
    assert b"thin" in pkg.lib().sm_last_error()
    # the span form (ragged k) needs a residual that follows D: a misaligned R is "not taken"
    res = _ep(pkg, act=RELU, R=0x1008, strideR=64)
    assert _fused(pkg, sfx, res, m=8, n=8, k=100, beta=1.0) == NOT_SUPPORTED


def test_python_holder_refuses_wrong_dtypes(pkg):
    torch = pytest.importorskip("torch")
    bias = torch.zeros(8, dtype=torch.float32)
    for bad in (bias.double(), bias.half(), bias.bfloat16(), bias.to(torch.int32)):
        with pytest.raises(pkg.SparsifymeError, match="bias is float32"):
            pkg.Epilogue(bias=bad)
    with pytest.raises(pkg.SparsifymeError, match="bias_dim"):
        pkg.Epilogue(bias=bias, bias_dim="depth")
    with pytest.raises(pkg.SparsifymeError, match="unknown activation"):
        pkg.Epilogue(act="gelu")
    e = pkg.Epilogue(bias=bias, bias_dim="row", act="relu6")
    assert (e.bias_dim, e.act, e.act_arg) == (ROW, CLIPPED, 6.0)
    assert pkg.Epilogue(act="leaky_relu", act_arg=0.1).act == LEAKY and pkg.Epilogue(act="hardswish").act == HARDSWISH
    # the residual has the output's dtype; refused before any pointer is taken (all of these are host tensors)
    D16 = torch.zeros(64, dtype=torch.float16)
    for bad_r in (D16.float(), D16.bfloat16(), D16.to(torch.int16)):
        ep = pkg.Epilogue(residual=bad_r)
        with pytest.raises(pkg.SparsifymeError, match="residual is"):
            pkg.spmma(D16, D16, D16, 8, 8, 64, beta=1.0, epilogue=ep)
        with pytest.raises(pkg.SparsifymeError, match="residual is"):
            pkg.spmma_fused(D16, D16, D16, 8, 8, 64, beta=1.0, epilogue=ep)
