"""The token-major fp8 2:4 weight-sparse linear layer (sm_linear24_fp8, sm_linear24_fp8_form) without a GPU: both symbols are declared,
exported and bound with the right arity; every argument-error and not-supported status is returned before any device work (fake
pointers, never dereferenced) with its sm_last_error text, an invalid epilogue before the shape is looked at; the dispatch rule as the
host-side query states it at 256 compute units -- every row of the layer table at every token count of the timing table, both sides of
every threshold, the empty and not-taken answers, and each tile form against the rule restated here; the Python wrapper's dtype checks."""
import csv
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
BIG = 1 << 31
E4M3, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2
RELU, CLIPPED = 1, 2
TOKENS = [1, 8, 16, 32, 64, 128, 512, 2048, 8192]
CUS = 256
FORMS = ("not_taken", "empty", "decode", "tile64", "tile128x64", "tile128")


def table():
    lines = open(os.path.join(ROOT, "datasets", "linear_shapes.csv")).read().splitlines()
    return [(int(r["out"]), int(r["in"])) for r in csv.DictReader(l for l in lines if not l.startswith("#"))]


def test_symbols_exported_declared_and_bound(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("sm_linear24_fp8", "sm_linear24_fp8_form"):
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    # blob, X, Y, tokens, out_features, in_features, ldx, ldy, fmt_w, fmt_x, out_type, alpha, beta, w_scale, x_scale, epilogue, stream
    sig = pkg._SIGS["sm_linear24_fp8"]
    assert len(sig) == 17
    assert sig[3:8] == [ctypes.c_size_t] * 5 and sig[8:11] == [ctypes.c_int] * 3 and sig[11:13] == [ctypes.c_float] * 2
    # tokens, out_features, in_features, cus, form
    assert len(pkg._SIGS["sm_linear24_fp8_form"]) == 5 and pkg._SIGS["sm_linear24_fp8_form"][:4] == [ctypes.c_size_t] * 4
    for i, name in enumerate(("NOT_TAKEN", "EMPTY", "DECODE", "TILE64", "TILE128x64", "TILE128")):
        assert f"#define SM_LINEAR24_FORM_{name} {i}\n" in header
    assert pkg.LINEAR24_FORMS == FORMS
    assert callable(pkg.linear24_fp8) and callable(pkg.linear24_fp8_form)


def _ep(pkg, bias=None, bias_dim=0, act=0, act_arg=0.0, R=None, strideR=0):
    st = pkg.EpilogueStruct()
    st.bias, st.bias_dim, st.act, st.act_arg, st.R, st.strideR = bias, bias_dim, act, act_arg, R, strideR
    return st


def _call(pkg, ep=None, blob=P, X=P, Y=P, tokens=8, out=8, inf=64, ldx=None, ldy=None, fw=E4M3, fx=E4M3, ot=BF16, beta=0.0, ws=None, xs=None):
    ldx = inf if ldx is None else ldx
    ldy = out if ldy is None else ldy
    return pkg.lib().sm_linear24_fp8(blob, X, Y, tokens, out, inf, ldx, ldy, fw, fx, ot, 1.0, beta, ws, xs,
                                     ctypes.addressof(ep) if ep is not None else None, None)


def _err(pkg):
    return pkg.lib().sm_last_error()


BAD_EPILOGUES = [
    (dict(act=5), 0.0), (dict(act=-1), 0.0), (dict(bias_dim=2), 0.0), (dict(bias_dim=-1), 0.0),
    (dict(act=RELU), 0.5),                                   # beta != 0 and no residual operand
    (dict(bias=0x3000, R=None), 1.0),
    (dict(act=CLIPPED, act_arg=-1.0), 0.0), (dict(act=CLIPPED, act_arg=float("inf")), 0.0), (dict(act=CLIPPED, act_arg=float("nan")), 0.0),
]


def test_invalid_epilogues_are_refused_before_everything_else(pkg):
    for kw, beta in BAD_EPILOGUES:
        assert _call(pkg, _ep(pkg, **kw), beta=beta) == INVALID, (kw, beta)
        assert b"sm_linear24_fp8: invalid epilogue" in _err(pkg)
        # ... on a shape that is not taken, on an empty one, and on arguments that are invalid themselves
        assert _call(pkg, _ep(pkg, **kw), beta=beta, inf=96, ldx=96) == INVALID and b"invalid epilogue" in _err(pkg)
        assert _call(pkg, _ep(pkg, **kw), beta=beta, tokens=0) == INVALID and b"invalid epilogue" in _err(pkg)
        assert _call(pkg, _ep(pkg, **kw), beta=beta, tokens=BIG) == INVALID and b"invalid epilogue" in _err(pkg)
        assert _call(pkg, _ep(pkg, **kw), beta=beta, blob=None, fw=7) == INVALID and b"invalid epilogue" in _err(pkg)


def test_statuses_before_any_device_work(pkg):
    for ep in (None, _ep(pkg), _ep(pkg, act=RELU)):
        for kw in (dict(blob=None), dict(X=None), dict(Y=None),
                   dict(blob=ODD),                                       # the blob is 16-byte aligned, as sm_spmma_fp8 asks
                   dict(fw=2), dict(fw=-1), dict(fx=2), dict(fx=-1), dict(ot=3), dict(ot=-1),
                   dict(ldx=63),                                         # ldx < in_features
                   dict(ldy=7)):                                         # ldy < out_features
            assert _call(pkg, ep, **kw) == INVALID, kw
            assert b"sm_linear24_fp8: invalid argument" in _err(pkg), kw
        # invalid arguments are answered before the not-supported shapes
        assert _call(pkg, ep, inf=96, ldx=95) == INVALID
        for kw, text in ((dict(inf=96, ldx=96), b"in_features"), (dict(inf=32, ldx=32), b"in_features"),
                         (dict(X=ODD), b"16-byte aligned rows of X"),    # X rows not 16-byte aligned: the pointer ...
                         (dict(ldx=72), b"16-byte aligned rows of X"),   # ... or the leading dimension
                         (dict(tokens=BIG), b"2^31"), (dict(out=BIG, ldy=BIG), b"2^31"), (dict(inf=BIG, ldx=BIG), b"2^31")):
            assert _call(pkg, ep, **kw) == NOT_SUPPORTED, kw
            assert b"sm_linear24_fp8" in _err(pkg) and text in _err(pkg), kw
        # every format pair and output type is a valid argument: an empty call succeeds with nothing enqueued, pointers untouched
        for fw in (E4M3, E5M2):
            for fx in (E4M3, E5M2):
                for ot in (F32, F16, BF16):
                    assert _call(pkg, ep, tokens=0, fw=fw, fx=fx, ot=ot) == 0
                    assert _call(pkg, ep, out=0, fw=fw, fx=fx, ot=ot) == 0
        # ... but not on a shape that is not taken
        assert _call(pkg, ep, tokens=0, inf=96, ldx=96) == NOT_SUPPORTED


def form(pkg, tokens, out, inf, cus=CUS):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_linear24_fp8_form(tokens, out, inf, cus, ctypes.byref(f)) == 0
    assert pkg.linear24_fp8_form(tokens, out, inf, cus=cus) == FORMS[f.value]
    return FORMS[f.value]


def want_tile(tokens, out, cus=CUS):
    """The rule restated: of 128 x 128, 128 x 64 and 64 x 64 (out features x tokens per workgroup) the largest tile whose grid still
    has at least `cus` workgroups; a 128-token tile is no larger than a 64-token one when there are at most 64 tokens."""
    up = lambda a, b: -(-a // b)
    if tokens > 64 and up(out, 128) * up(tokens, 128) >= cus:
        return "tile128"
    if up(out, 128) * up(tokens, 64) >= cus:
        return "tile128x64"
    return "tile64"


def test_form_query_statuses_empty_and_not_taken(pkg):
    assert pkg.lib().sm_linear24_fp8_form(8, 8, 64, CUS, None) == INVALID
    assert b"sm_linear24_fp8_form" in _err(pkg)
    for tokens, out in ((0, 8), (8, 0), (0, 0)):
        assert form(pkg, tokens, out, 64) == "empty"
        assert form(pkg, tokens, out, 0) == "empty"
    # what the entry point answers SM_STATUS_NOT_SUPPORTED to, the empty shapes among them (the entry point looks at the shape first)
    for tokens, out, inf in ((8, 8, 96), (8, 8, 32), (8, 8, 100), (0, 8, 96), (BIG, 8, 64), (8, BIG, 64), (8, 8, BIG), (0, BIG, 64)):
        assert form(pkg, tokens, out, inf) == "not_taken", (tokens, out, inf)
        if inf < BIG:
            assert _call(pkg, None, tokens=tokens, out=out, inf=inf, ldy=out) == NOT_SUPPORTED
    assert form(pkg, BIG - 1, 8, 64) != "not_taken" and form(pkg, 8, BIG - 1, 64) != "not_taken" and form(pkg, 8, 8, BIG - 64) != "not_taken"


def test_a_tile_grid_beyond_the_launch_limit_is_not_taken(pkg):
    """Dimensions below 2^31 whose tile count passes 2^31 - 1 workgroups: the query says not_taken, as the entry point refuses them."""
    out = 128 << 16
    assert form(pkg, (128 << 15) - 128, out, 64) == "tile128"          # (2^15 - 1) * 2^16 workgroups of 128 x 128
    for tokens, o in ((128 << 15, out), (BIG - 1, BIG - 1)):
        assert form(pkg, tokens, o, 64) == "not_taken", (tokens, o)
        assert _call(pkg, None, tokens=tokens, out=o) == NOT_SUPPORTED
        assert b"sm_linear24_fp8: grid too large" in _err(pkg)


def decode_limits(pkg):
    """The decode form's thresholds, read from the query itself: the largest token count it takes (at a small out), and the largest out
    (at one token).  Both are found by bisection over a monotone answer, which is asserted at the ends."""
    def last_true(f, lo, hi):
        assert f(lo) and not f(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if f(mid) else (lo, mid)
        return lo
    tmax = last_true(lambda t: form(pkg, t, 4096, 4096) == "decode", 1, 1 << 20)
    omax = last_true(lambda o: form(pkg, 1, o, 4096) == "decode", 1, 1 << 30)
    return tmax, omax


def test_form_rule_on_the_layer_table_and_at_every_threshold(pkg):
    tmax, omax = decode_limits(pkg)
    assert 1 <= tmax < 128 and omax >= 4096
    seen = set()
    for out, inf in table():
        for tokens in TOKENS:
            got = form(pkg, tokens, out, inf)
            want = "decode" if tokens <= tmax and out <= omax else want_tile(tokens, out)
            assert got == want, (tokens, out, inf, got, want)
            seen.add(got)
    assert seen == {"decode", "tile64", "tile128x64", "tile128"}
    # both sides of the decode thresholds; in_features plays no part in the rule
    for inf in (64, 4096, 14336):
        assert form(pkg, tmax, omax, inf) == "decode" and form(pkg, 1, 1, inf) == "decode"
        assert form(pkg, tmax + 1, omax, inf) == want_tile(tmax + 1, omax)
        assert form(pkg, tmax, omax + 1, inf) == want_tile(tmax, omax + 1)
        assert form(pkg, 1, omax + 1, inf) == want_tile(1, omax + 1)
    # both sides of the tile thresholds: 256 workgroups of 128 x 128, of 128 x 64, and the 64-token limit of the 128-token tile
    for tokens, out in ((256, 128 * 128), (256, 128 * 127 + 1), (256, 128 * 127), (129, 128 * 128), (128, 128 * 256), (128, 128 * 255),
                        (65, 128 * 256), (64, 128 * 256), (64, 128 * 255 + 1), (64, 128 * 255), (32, 128 * 256), (32, 128 * 255),
                        (2048, 128 * 16), (2048, 128 * 15 + 1), (2048, 128 * 15), (2048, 128 * 8), (2048, 128 * 7 + 1), (2048, 128 * 7), (17, 64), (17, 1)):
        if tokens <= tmax and out <= omax:
            continue
        assert form(pkg, tokens, out, 128) == want_tile(tokens, out), (tokens, out)
    assert form(pkg, 256, 128 * 128, 128) == "tile128" and form(pkg, 256, 128 * 127, 128) == "tile128x64"
    assert form(pkg, 128, 128 * 128, 128) == "tile128x64" and form(pkg, 128, 128 * 127, 128) == "tile64"
    assert form(pkg, 65, 128 * 256, 128) == "tile128" and form(pkg, 64, 128 * 256, 128) == "tile128x64" and form(pkg, 64, 128 * 255, 128) == "tile64"
    # the tile rule follows the compute-unit count it is asked about
    assert form(pkg, 256, 128 * 64, 128, cus=128) == "tile128" and form(pkg, 256, 128 * 64, 128, cus=129) == "tile128x64"
    assert form(pkg, 256, 128 * 64, 128, cus=257) == "tile64"


def test_python_wrapper_refuses_wrong_dtypes(pkg):
    torch = pytest.importorskip("torch")
    x8 = torch.zeros(64, dtype=torch.uint8).view(torch.float8_e4m3fn)
    h, f, i32 = torch.zeros(64, dtype=torch.float16), torch.zeros(64, dtype=torch.float32), torch.zeros(64, dtype=torch.int32)
    blob = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(pkg.SparsifymeError, match="float8"):
        pkg.linear24_fp8(blob, h, h, 1, 1, 64)                        # X is not fp8
    with pytest.raises(pkg.SparsifymeError, match="float8"):
        pkg.linear24_fp8(blob, x8, h, 1, 1, 64, w_dtype=torch.int8)
    with pytest.raises(pkg.SparsifymeError, match="float32, float16 or bfloat16"):
        pkg.linear24_fp8(blob, x8, i32, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="w_scale is float32"):
        pkg.linear24_fp8(blob, x8, h, 1, 1, 64, w_scale=h)
    with pytest.raises(pkg.SparsifymeError, match="x_scale is float32"):
        pkg.linear24_fp8(blob, x8, h, 1, 1, 64, x_scale=h)
    # the residual has Y's dtype; refused before any pointer is taken (host tensors throughout)
    with pytest.raises(pkg.SparsifymeError, match="residual is"):
        pkg.linear24_fp8(blob, x8, h, 1, 1, 64, beta=1.0, epilogue=pkg.Epilogue(residual=f))
