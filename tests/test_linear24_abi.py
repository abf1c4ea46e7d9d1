"""The token-major 2:4 weight-sparse linear layer (sm_linear24_{f16,bf16}) without a GPU: both symbols are declared, exported and
bound with the right arity; every argument-error and not-supported status is returned before any device work (fake pointers, never
dereferenced), an invalid epilogue before the shape is looked at; the Python wrapper refuses wrong or mixed dtypes before it takes
a pointer; the shape table parses."""
import csv
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sm_linear24_f16", "sm_linear24_bf16"]
INVALID, NOT_SUPPORTED = 1, 2
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
BIG = 1 << 31
SFX = ["f16", "bf16"]
RELU, CLIPPED = 1, 2
TABLE = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (12288, 4096), (22016, 4096), (4096, 11008)]


def test_symbols_exported_declared_and_bound(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        # blob, X, Y, tokens, out_features, in_features, ldx, ldy, alpha, beta, epilogue, stream
        assert len(pkg._SIGS[name]) == 12
        assert pkg._SIGS[name][3:8] == [ctypes.c_size_t] * 5 and pkg._SIGS[name][8:10] == [ctypes.c_float] * 2
    assert callable(pkg.linear24)


def _ep(pkg, bias=None, bias_dim=0, act=0, act_arg=0.0, R=None, strideR=0):
    st = pkg.EpilogueStruct()
    st.bias, st.bias_dim, st.act, st.act_arg, st.R, st.strideR = bias, bias_dim, act, act_arg, R, strideR
    return st


def _call(pkg, sfx, ep=None, blob=P, X=P, Y=P, tokens=8, out=8, inf=64, ldx=None, ldy=None, beta=0.0):
    fn = getattr(pkg.lib(), "sm_linear24_" + sfx)
    ldx = inf if ldx is None else ldx
    ldy = out if ldy is None else ldy
    return fn(blob, X, Y, tokens, out, inf, ldx, ldy, 1.0, beta, ctypes.addressof(ep) if ep is not None else None, None)


BAD_EPILOGUES = [
    (dict(act=5), 0.0), (dict(act=-1), 0.0), (dict(bias_dim=2), 0.0), (dict(bias_dim=-1), 0.0),
    (dict(act=RELU), 0.5),                                   # beta != 0 and no residual operand
    (dict(bias=0x3000, R=None), 1.0),
    (dict(act=CLIPPED, act_arg=-1.0), 0.0), (dict(act=CLIPPED, act_arg=float("inf")), 0.0), (dict(act=CLIPPED, act_arg=float("nan")), 0.0),
]


@pytest.mark.parametrize("sfx", SFX)
def test_invalid_epilogues_are_refused_before_the_shape(pkg, sfx):
    for kw, beta in BAD_EPILOGUES:
        assert _call(pkg, sfx, _ep(pkg, **kw), beta=beta) == INVALID, (kw, beta)
        assert b"invalid epilogue" in pkg.lib().sm_last_error()
        # ... on a shape that is not taken, and on an empty one
        assert _call(pkg, sfx, _ep(pkg, **kw), beta=beta, inf=96, ldx=96) == INVALID
        assert _call(pkg, sfx, _ep(pkg, **kw), beta=beta, tokens=0) == INVALID


@pytest.mark.parametrize("sfx", SFX)
def test_statuses_before_any_device_work(pkg, sfx):
    for ep in (None, _ep(pkg), _ep(pkg, act=RELU)):
        assert _call(pkg, sfx, ep, blob=None) == INVALID
        assert _call(pkg, sfx, ep, X=None) == INVALID
        assert _call(pkg, sfx, ep, blob=ODD) == INVALID          # the blob is 16-byte aligned, as sm_spmma_* asks
        assert _call(pkg, sfx, ep, Y=None) == INVALID
        assert _call(pkg, sfx, ep, ldx=63) == INVALID            # ldx < in_features
        assert _call(pkg, sfx, ep, ldy=7) == INVALID             # ldy < out_features
        assert _call(pkg, sfx, ep, inf=96, ldx=96) == NOT_SUPPORTED
        assert _call(pkg, sfx, ep, inf=32, ldx=32) == NOT_SUPPORTED
        assert _call(pkg, sfx, ep, X=ODD) == NOT_SUPPORTED       # X rows not 16-byte aligned: the pointer ...
        assert _call(pkg, sfx, ep, ldx=68) == NOT_SUPPORTED      # ... or the leading dimension
        assert _call(pkg, sfx, ep, tokens=BIG) == NOT_SUPPORTED
        assert _call(pkg, sfx, ep, out=BIG, ldy=BIG) == NOT_SUPPORTED
        assert _call(pkg, sfx, ep, inf=BIG, ldx=BIG) == NOT_SUPPORTED
        # nothing to do: success, nothing enqueued, pointers untouched
        assert _call(pkg, sfx, ep, tokens=0) == 0
        assert _call(pkg, sfx, ep, out=0) == 0


def test_python_wrapper_refuses_wrong_and_mixed_dtypes(pkg):
    torch = pytest.importorskip("torch")
    h, b, f = torch.zeros(64, dtype=torch.float16), torch.zeros(64, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.float32)
    blob = torch.zeros(64, dtype=torch.uint8)
    for X, Y in ((h, b), (b, h), (f, f), (h, f), (f, h)):
        with pytest.raises(pkg.SparsifymeError, match="linear24: X and Y"):
            pkg.linear24(blob, X, Y, 1, 1, 64)
    # the residual has Y's dtype; refused before any pointer is taken (host tensors throughout)
    with pytest.raises(pkg.SparsifymeError, match="residual is"):
        pkg.linear24(blob, h, h, 1, 1, 64, beta=1.0, epilogue=pkg.Epilogue(residual=b))


def test_shape_table():
    path = os.path.join(ROOT, "datasets", "linear_shapes.csv")
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#")
    rows = list(csv.DictReader(l for l in lines if not l.startswith("#")))
    assert [(int(r["out"]), int(r["in"])) for r in rows] == TABLE
    for r in rows:
        assert int(r["in"]) % 64 == 0 and int(r["count"]) >= 1
