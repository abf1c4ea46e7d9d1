"""The gated (gate/up) token-major 2:4 layers (sm_linear24_glu_{f16,bf16,fp8}, sm_linear24_glu_form) without a GPU: the symbols are
declared, exported and bound with the right arity; every argument-error and not-supported status is returned before any device work
(fake pointers, never dereferenced), in the documented order, with a text that names the entry point; the form query IS the plain
layer's rule on 2 * hidden rows -- on a grid, at both sides of every threshold and at the hidden limit; the wrappers' dtype checks."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
BIG = 1 << 31
HMAX = 0x3fffffff                 # the largest hidden: 2 * hidden is still a 31-bit row count
E4M3, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2
NONE, RELU, SILU = 0, 1, 2
FORMS = ("not_taken", "empty", "decode", "tile64", "tile128x64", "tile128")
NAMES16 = ("sm_linear24_glu_f16", "sm_linear24_glu_bf16")
WHO16, WHO8 = b"sm_linear24_glu_{f16,bf16}", b"sm_linear24_glu_fp8"


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sparsifyme.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sm_[a-z0-9_]+)\s*\(", src)))


def test_symbols_exported_declared_and_bound(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES16 + ("sm_linear24_glu_fp8", "sm_linear24_glu_form"):
        assert name + "(" in header
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    assert declared_symbols() == pkg.EXPORTED_SYMBOLS
    for name in NAMES16:   # blob, X, Y, tokens, hidden, in_features, ldx, ldy, act, bias, stream
        sig = pkg._SIGS[name]
        assert len(sig) == 11 and sig[3:8] == [ctypes.c_size_t] * 5 and sig[8] == ctypes.c_int
    # blob, X, Y, tokens, hidden, in_features, ldx, ldy, fmt_w, fmt_x, out_type, act, w_scale, x_scale, bias, stream
    sig = pkg._SIGS["sm_linear24_glu_fp8"]
    assert len(sig) == 16 and sig[3:8] == [ctypes.c_size_t] * 5 and sig[8:12] == [ctypes.c_int] * 4
    assert len(pkg._SIGS["sm_linear24_glu_form"]) == 5 and pkg._SIGS["sm_linear24_glu_form"][:4] == [ctypes.c_size_t] * 4
    for i, name in enumerate(("NONE", "RELU", "SILU")):
        assert re.search(r"#define SM_GLU_ACT_%s %d\b" % (name, i), header)
    assert pkg.GLU_ACTS == {"none": NONE, "relu": RELU, "silu": SILU}
    assert callable(pkg.linear24_glu) and callable(pkg.linear24_glu_fp8) and callable(pkg.linear24_glu_form)


def call16(pkg, name="sm_linear24_glu_f16", blob=P, X=P, Y=P, tokens=8, hidden=8, inf=64, ldx=None, ldy=None, act=SILU, bias=None):
    ldx = inf if ldx is None else ldx
    ldy = hidden if ldy is None else ldy
    return getattr(pkg.lib(), name)(blob, X, Y, tokens, hidden, inf, ldx, ldy, act, bias, None)


def call8(pkg, blob=P, X=P, Y=P, tokens=8, hidden=8, inf=64, ldx=None, ldy=None, fw=E4M3, fx=E4M3, ot=BF16, act=SILU, ws=None, xs=None, bias=None):
    ldx = inf if ldx is None else ldx
    ldy = hidden if ldy is None else ldy
    return pkg.lib().sm_linear24_glu_fp8(blob, X, Y, tokens, hidden, inf, ldx, ldy, fw, fx, ot, act, ws, xs, bias, None)


def _err(pkg):
    return pkg.lib().sm_last_error()


def callers(pkg):
    """(call, the name its messages carry, elements of X per 16 bytes)"""
    return [(lambda n=n, **kw: call16(pkg, n, **kw), WHO16, 8) for n in NAMES16] + [(lambda **kw: call8(pkg, **kw), WHO8, 16)]


def test_statuses_before_any_device_work_in_their_order(pkg):
    for call, who, per16 in callers(pkg):
        # 1. the activation, before everything else: on invalid arguments, on a shape that is not taken, on an empty one
        for act in (-1, 3, 7):
            for kw in (dict(), dict(blob=None), dict(ldy=7), dict(inf=96, ldx=96), dict(tokens=0), dict(tokens=BIG), dict(hidden=HMAX + 1, ldy=BIG)):
                assert call(act=act, **kw) == INVALID, (act, kw)
                assert who in _err(pkg) and b"act is not SM_GLU_ACT_*" in _err(pkg), (act, kw)
        for act in (NONE, RELU, SILU):
            # 2. the plain layer's invalid arguments, with ldy read on hidden
            for kw in (dict(blob=None), dict(X=None), dict(Y=None), dict(blob=ODD), dict(ldx=63), dict(ldy=7)):
                assert call(act=act, **kw) == INVALID, kw
                assert who + b": invalid argument" in _err(pkg) and b"ldy < hidden" in _err(pkg), kw
            # ... answered before the not-supported shapes
            assert call(act=act, inf=96, ldx=95) == INVALID and call(act=act, tokens=BIG, ldy=7) == INVALID
            assert call(act=act, hidden=HMAX + 1, ldy=HMAX) == INVALID
            # 3. dimensions: 2^31 and beyond, and a hidden whose 2 * hidden does not fit
            for kw in (dict(tokens=BIG), dict(inf=BIG, ldx=BIG), dict(hidden=BIG, ldy=BIG), dict(hidden=HMAX + 1, ldy=HMAX + 1)):
                assert call(act=act, **kw) == NOT_SUPPORTED, kw
                assert who in _err(pkg) and b"2^31" in _err(pkg), kw
            # ... before 4.: in_features % 64 and the alignment of X's rows
            assert call(act=act, tokens=BIG, inf=96, ldx=96) == NOT_SUPPORTED and b"2^31" in _err(pkg)
            for kw, text in ((dict(inf=96, ldx=96), b"in_features"), (dict(inf=32, ldx=32), b"in_features"),
                             (dict(X=ODD), b"16-byte aligned rows of X"), (dict(ldx=64 + per16 // 2), b"16-byte aligned rows of X")):
                assert call(act=act, **kw) == NOT_SUPPORTED, kw
                assert who in _err(pkg) and text in _err(pkg), kw
            # 5. empty: success, nothing enqueued, pointers untouched -- but not on a shape that is not taken
            assert call(act=act, tokens=0) == 0 and call(act=act, hidden=0, ldy=0) == 0 and call(act=act, tokens=0, hidden=0) == 0
            assert call(act=act, tokens=0, inf=96, ldx=96) == NOT_SUPPORTED
            assert call(act=act, tokens=0, hidden=HMAX, ldy=HMAX) == 0 and call(act=act, tokens=0, hidden=HMAX + 1, ldy=HMAX + 1) == NOT_SUPPORTED


def test_fp8_formats_and_output_types(pkg):
    for kw in (dict(fw=2), dict(fw=-1), dict(fx=2), dict(fx=-1), dict(ot=3), dict(ot=-1)):
        assert call8(pkg, **kw) == INVALID, kw
        assert WHO8 + b": invalid argument" in _err(pkg) and b"fmt not SM_FP8_*" in _err(pkg), kw
        assert call8(pkg, act=5, **kw) == INVALID and b"act is not" in _err(pkg)
    for fw in (E4M3, E5M2):
        for fx in (E4M3, E5M2):
            for ot in (F32, F16, BF16):
                assert call8(pkg, tokens=0, fw=fw, fx=fx, ot=ot) == 0


def test_a_tile_grid_beyond_the_launch_limit_is_not_supported(pkg):
    """Dimensions inside their limits whose tile count passes 2^31 - 1 workgroups."""
    hidden = 64 << 16                                   # 2^16 tiles of 128 blob rows
    assert glu_form(pkg, (128 << 15) - 128, hidden, 64, 256) == "tile128"
    for tokens, h in ((128 << 15, hidden), (BIG - 1, HMAX)):
        assert glu_form(pkg, tokens, h, 64, 256) == "not_taken"
        assert call16(pkg, tokens=tokens, hidden=h) == NOT_SUPPORTED and WHO16 + b": grid too large" in _err(pkg)
        assert call8(pkg, tokens=tokens, hidden=h) == NOT_SUPPORTED and WHO8 + b": grid too large" in _err(pkg)


def glu_form(pkg, tokens, hidden, inf, cus):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_linear24_glu_form(tokens, hidden, inf, cus, ctypes.byref(f)) == 0
    assert pkg.linear24_glu_form(tokens, hidden, inf, cus=cus) == FORMS[f.value]
    return FORMS[f.value]


def plain_form(pkg, tokens, out, inf, cus):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_linear24_fp8_form(tokens, out, inf, cus, ctypes.byref(f)) == 0
    return FORMS[f.value]


def test_form_query_is_the_plain_rule_on_twice_hidden(pkg):
    assert pkg.lib().sm_linear24_glu_form(8, 8, 64, 256, None) == INVALID
    assert b"sm_linear24_glu_form" in _err(pkg)
    seen = set()

    def same(tokens, hidden, inf, cus):
        got = glu_form(pkg, tokens, hidden, inf, cus)
        assert got == plain_form(pkg, tokens, 2 * hidden, inf, cus), (tokens, hidden, inf, cus)
        seen.add(got)
        return got

    # a grid, the two gate/up rows of the layer table among it
    for tokens in (0, 1, 8, 16, 17, 32, 64, 65, 128, 512, 2048, 8192):
        for hidden in (0, 1, 16, 65, 2048, 4099, 8192, 8193, 11008, 14336, 1 << 20):
            for inf in (64, 96, 4096):
                for cus in (1, 128, 256, 304):
                    same(tokens, hidden, inf, cus)
    assert seen == set(FORMS)
    # both sides of every threshold: tokens 16 / 17 (decode) and 64 / 65 (the 128-token tile), 2 hidden 16384 / 16386
    assert same(16, 8192, 64, 256) == "decode" and same(17, 8192, 64, 256) != "decode"
    assert same(16, 8193, 64, 256) != "decode" and same(1, 8193, 64, 256) != "decode" and same(1, 8192, 64, 256) == "decode"
    assert same(65, 64 * 256, 128, 256) == "tile128" and same(64, 64 * 256, 128, 256) == "tile128x64"
    # the cus boundary of each tile: a tile of 128 blob rows is 64 hidden features
    for cus in (128, 256, 304):
        assert same(256, 64 * (cus // 2), 128, cus) == "tile128"            # ceil(2h / 128) * 2 == cus workgroups of 128 x 128
        assert same(256, 64 * (cus // 2) - 1, 128, cus) == "tile128"        # (the same tile count)
        assert same(256, 64 * (cus // 2 - 1), 128, cus) == "tile128x64"     # one tile row fewer: cus - 2 of them, 2 cus - 4 of 128 x 64
        assert same(128, 64 * (cus // 2), 128, cus) == "tile128x64"
        assert same(128, 64 * (cus // 2 - 1), 128, cus) == "tile64"
        assert same(64, 64 * cus, 128, cus) == "tile128x64" and same(64, 64 * (cus - 1), 128, cus) == "tile64"
    assert same(256, 64 * 64, 128, 129) == "tile128x64" and same(256, 64 * 64, 128, 257) == "tile64"
    # the hidden limit: 2 * hidden must fit the 31-bit row count
    assert same(8, HMAX, 64, 256) != "not_taken" and same(8, HMAX + 1, 64, 256) == "not_taken"
    assert glu_form(pkg, 8, BIG, 64, 256) == "not_taken" and glu_form(pkg, 0, HMAX + 1, 64, 256) == "not_taken"
    assert glu_form(pkg, 8, 1 << 63, 64, 256) == "not_taken"              # 2 * hidden would wrap to 0 (= empty) in 64 bits
    # cus = 0 asks the device (256 when none is visible): a valid answer either way
    assert glu_form(pkg, 300, 8196, 192, 0) in FORMS[3:]


def test_python_wrappers_refuse_wrong_dtypes_and_acts(pkg):
    torch = pytest.importorskip("torch")
    x8 = torch.zeros(64, dtype=torch.uint8).view(torch.float8_e4m3fn)
    h, b, f, i32 = torch.zeros(64, dtype=torch.float16), torch.zeros(64, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.float32), torch.zeros(64, dtype=torch.int32)
    blob = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(pkg.SparsifymeError, match="both float16 or both bfloat16"):
        pkg.linear24_glu(blob, h, b, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="both float16 or both bfloat16"):
        pkg.linear24_glu(blob, f, f, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="act is one of"):
        pkg.linear24_glu(blob, h, h, 1, 1, 64, act="gelu")
    with pytest.raises(pkg.SparsifymeError, match="bias is float32"):
        pkg.linear24_glu(blob, h, h, 1, 1, 64, bias=h)
    with pytest.raises(pkg.SparsifymeError, match="float8"):
        pkg.linear24_glu_fp8(blob, h, h, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="float32, float16 or bfloat16"):
        pkg.linear24_glu_fp8(blob, x8, i32, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="act is one of"):
        pkg.linear24_glu_fp8(blob, x8, h, 1, 1, 64, act="hardswish")
    with pytest.raises(pkg.SparsifymeError, match="w_scale is float32"):
        pkg.linear24_glu_fp8(blob, x8, h, 1, 1, 64, w_scale=h)
    with pytest.raises(pkg.SparsifymeError, match="x_scale is float32"):
        pkg.linear24_glu_fp8(blob, x8, h, 1, 1, 64, x_scale=h)
    with pytest.raises(pkg.SparsifymeError, match="bias is float32"):
        pkg.linear24_glu_fp8(blob, x8, h, 1, 1, 64, bias=h)
