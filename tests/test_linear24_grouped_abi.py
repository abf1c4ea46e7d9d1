"""The grouped (per-expert) token-major 2:4 layers (sm_linear24_grouped_{f16,bf16,fp8}, sm_linear24_grouped_glu_{f16,bf16,fp8},
sm_linear24_grouped_form) without a GPU: the seven symbols are declared, exported and bound with the right arity; every
argument-error and not-supported status is returned before any device work (fake pointers, never dereferenced), in the documented
order, with a text that names the entry point; the form query against the rule restated here -- at both sides of every threshold,
at the group limit, the groups * out limit and the grid limit read on tiles_m * slots; the slot bound against brute force."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
P = ctypes.c_void_p(0x1000)       # 16-byte aligned stand-in for a device pointer
ODD = ctypes.c_void_p(0x1008)     # 8-byte aligned only
BIG = 1 << 31
LIM = BIG - 1
HMAX = 0x3fffffff
MAXG = 1024
E4M3, E5M2 = 0, 1
F32, F16, BF16 = 0, 1, 2
NONE, RELU, SILU = 0, 1, 2
FORMS = ("not_taken", "empty", "decode", "tile64", "tile128x64", "tile128")
PLAIN16 = ("sm_linear24_grouped_f16", "sm_linear24_grouped_bf16")
GLU16 = ("sm_linear24_grouped_glu_f16", "sm_linear24_grouped_glu_bf16")
SEVEN = PLAIN16 + ("sm_linear24_grouped_fp8",) + GLU16 + ("sm_linear24_grouped_glu_fp8", "sm_linear24_grouped_form")
WHO = {"p16": b"sm_linear24_grouped_{f16,bf16}", "p8": b"sm_linear24_grouped_fp8", "g16": b"sm_linear24_grouped_glu_{f16,bf16}",
       "g8": b"sm_linear24_grouped_glu_fp8"}


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sparsifyme.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sm_[a-z0-9_]+)\s*\(", src)))


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    for name in SEVEN:
        assert name + "(" in header, name
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in SEVEN:
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    assert declared_symbols() == pkg.EXPORTED_SYMBOLS
    sz, ci, cf = ctypes.c_size_t, ctypes.c_int, ctypes.c_float
    for name in PLAIN16:  # blob, X, Y, group_offsets, groups, tokens, out, in, ldx, ldy, alpha, beta, epilogue, stream
        sig = pkg._SIGS[name]
        assert len(sig) == 14 and sig[4:10] == [sz] * 6 and sig[10:12] == [cf] * 2
    sig = pkg._SIGS["sm_linear24_grouped_fp8"]  # ... ldy, fmt_w, fmt_x, out_type, alpha, beta, w_scale, x_scale, epilogue, stream
    assert len(sig) == 19 and sig[4:10] == [sz] * 6 and sig[10:13] == [ci] * 3 and sig[13:15] == [cf] * 2
    for name in GLU16:    # blob, X, Y, group_offsets, groups, tokens, hidden, in, ldx, ldy, act, bias, stream
        sig = pkg._SIGS[name]
        assert len(sig) == 13 and sig[4:10] == [sz] * 6 and sig[10] == ci
    sig = pkg._SIGS["sm_linear24_grouped_glu_fp8"]  # ... ldy, fmt_w, fmt_x, out_type, act, w_scale, x_scale, bias, stream
    assert len(sig) == 18 and sig[4:10] == [sz] * 6 and sig[10:14] == [ci] * 4
    assert len(pkg._SIGS["sm_linear24_grouped_form"]) == 6 and pkg._SIGS["sm_linear24_grouped_form"][:5] == [sz] * 5
    assert re.search(r"#define SM_LINEAR24_MAX_GROUPS %d\b" % MAXG, header) and pkg.LINEAR24_MAX_GROUPS == MAXG
    for fn in ("linear24_grouped", "linear24_grouped_fp8", "linear24_grouped_glu", "linear24_grouped_glu_fp8", "linear24_grouped_form"):
        assert callable(getattr(pkg, fn))


# every caller takes the same keywords; `out` is out_features or hidden
def p16(pkg, name="sm_linear24_grouped_f16", blob=P, X=P, Y=P, off=P, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, ep=None):
    return getattr(pkg.lib(), name)(blob, X, Y, off, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, 1.0, 0.0, ep, None)


def p8(pkg, blob=P, X=P, Y=P, off=P, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, fw=E4M3, fx=E4M3, ot=BF16, ep=None):
    return pkg.lib().sm_linear24_grouped_fp8(blob, X, Y, off, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, fw, fx, ot,
                                             1.0, 0.0, None, None, ep, None)


def g16(pkg, name="sm_linear24_grouped_glu_f16", blob=P, X=P, Y=P, off=P, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, act=SILU):
    return getattr(pkg.lib(), name)(blob, X, Y, off, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, act, None, None)


def g8(pkg, blob=P, X=P, Y=P, off=P, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, fw=E4M3, fx=E4M3, ot=BF16, act=SILU):
    return pkg.lib().sm_linear24_grouped_glu_fp8(blob, X, Y, off, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, fw, fx,
                                                 ot, act, None, None, None, None)


def _err(pkg):
    return pkg.lib().sm_last_error()


def callers(pkg):
    """(call, the name its messages carry, elements of X per 16 bytes, gated, rows of the blob per out feature of Y)"""
    return ([(lambda n=n, **kw: p16(pkg, n, **kw), WHO["p16"], 8, False) for n in PLAIN16] + [(lambda **kw: p8(pkg, **kw), WHO["p8"], 16, False)] +
            [(lambda n=n, **kw: g16(pkg, n, **kw), WHO["g16"], 8, True) for n in GLU16] + [(lambda **kw: g8(pkg, **kw), WHO["g8"], 16, True)])


class Epi(ctypes.Structure):   # sm_epilogue_t
    _fields_ = [("bias", ctypes.c_void_p), ("bias_dim", ctypes.c_int), ("act", ctypes.c_int), ("act_arg", ctypes.c_float), ("R", ctypes.c_void_p),
                ("strideR", ctypes.c_size_t)]


def test_statuses_before_any_device_work_in_their_order(pkg):
    for call, who, per16, gated in callers(pkg):
        rows = 2 if gated else 1                      # blob rows per feature of Y
        omax = HMAX if gated else LIM                 # the largest `out` of a single group
        others = (dict(), dict(blob=None), dict(off=None), dict(ldy=7), dict(inf=96, ldx=96), dict(tokens=0), dict(tokens=BIG), dict(groups=MAXG + 1))
        # 1. the epilogue (gated: the activation) before everything else
        if gated:
            for act in (-1, 3):
                for kw in others:
                    assert call(act=act, **kw) == INVALID, (act, kw)
                    assert who in _err(pkg) and b"act is not SM_GLU_ACT_*" in _err(pkg)
        else:
            bad = Epi(None, 5, 0, 0.0, None, 0)       # unknown bias_dim
            for kw in others:
                assert call(ep=ctypes.byref(bad), **kw) == INVALID, kw
                assert who + b": invalid epilogue" in _err(pkg)
        # 2. invalid arguments, the offsets among them
        for kw in (dict(blob=None), dict(X=None), dict(Y=None), dict(off=None), dict(blob=ODD), dict(ldx=63), dict(ldy=7)):
            assert call(**kw) == INVALID, kw
            assert who + b": invalid argument" in _err(pkg) and b"null group_offsets" in _err(pkg), kw
        # ... answered before the not-supported shapes
        assert call(inf=96, ldx=95) == INVALID and call(tokens=BIG, ldy=7) == INVALID and call(groups=MAXG + 1, off=None) == INVALID
        # 3. dimensions, the group limit, groups * rows
        for kw in (dict(tokens=BIG), dict(inf=BIG, ldx=BIG), dict(out=BIG, ldy=BIG), dict(out=omax + 1, ldy=omax + 1, groups=1)):
            assert call(**kw) == NOT_SUPPORTED, kw
            assert who in _err(pkg) and b"2^31" in _err(pkg), kw
        for kw in (dict(groups=MAXG + 1), dict(groups=1 << 40), dict(groups=2, out=omax // 2 + 1, ldy=omax), dict(groups=MAXG, out=omax // MAXG + 1, ldy=omax)):
            assert call(**kw) == NOT_SUPPORTED, kw
            assert who in _err(pkg) and b"SM_LINEAR24_MAX_GROUPS" in _err(pkg) and b"2^31" in _err(pkg), kw
        assert rows * (omax // MAXG) * MAXG <= LIM < rows * (omax // MAXG + 1) * MAXG
        # ... before 4.: in_features % 64 and the alignment of X's rows
        assert call(groups=MAXG + 1, inf=96, ldx=96) == NOT_SUPPORTED and b"SM_LINEAR24_MAX_GROUPS" in _err(pkg)
        for kw, text in ((dict(inf=96, ldx=96), b"in_features"), (dict(inf=32, ldx=32), b"in_features"), (dict(X=ODD), b"16-byte aligned rows of X"),
                         (dict(ldx=64 + per16 // 2), b"16-byte aligned rows of X")):
            assert call(**kw) == NOT_SUPPORTED, kw
            assert who in _err(pkg) and text in _err(pkg), kw
        # 5. empty: success, nothing enqueued, pointers untouched -- but not on a shape that is not taken
        assert call(tokens=0) == 0 and call(out=0, ldy=0) == 0 and call(groups=0) == 0 and call(groups=MAXG, tokens=0) == 0
        assert call(tokens=0, inf=96, ldx=96) == NOT_SUPPORTED and call(tokens=0, groups=MAXG + 1) == NOT_SUPPORTED
        assert call(groups=0, off=None) == INVALID
        # the grid limit, on dimensions inside their limits: tiles_m * slots
        out = (64 << 16) if gated else (128 << 16)     # 2^16 tile rows
        assert call(groups=1, tokens=LIM, out=out, ldy=out) == NOT_SUPPORTED and who + b": grid too large" in _err(pkg)


def test_fp8_formats_and_output_types(pkg):
    for call, who in ((lambda **kw: p8(pkg, **kw), WHO["p8"]), (lambda **kw: g8(pkg, **kw), WHO["g8"])):
        for kw in (dict(fw=2), dict(fw=-1), dict(fx=2), dict(fx=-1), dict(ot=3), dict(ot=-1)):
            assert call(**kw) == INVALID, kw
            assert who + b": invalid argument" in _err(pkg) and b"fmt not SM_FP8_*" in _err(pkg), kw
        for fw, fx, ot in itertools.product((E4M3, E5M2), (E4M3, E5M2), (F32, F16, BF16)):
            assert call(tokens=0, fw=fw, fx=fx, ot=ot) == 0


# ------------------------------------------------------------------------------------------------ the rule, restated
def cdiv(a, b):
    return -(-a // b)


def slots(tokens, groups, bn):
    return min(tokens, cdiv(tokens, bn) + groups - 1)


def rule(tokens, groups, out, inf, cus):
    if inf % 64 or tokens > LIM or out > LIM or inf > LIM or groups > MAXG or groups * out > LIM:
        return "not_taken"
    if tokens == 0 or out == 0 or groups == 0:
        return "empty"
    mean = cdiv(tokens, groups)
    if mean > 64 and cdiv(out, 128) * cdiv(tokens, 128) >= cus:
        form, bm, bn = "tile128", 128, 128
    elif cdiv(out, 128) * cdiv(tokens, 64) >= cus:
        form, bm, bn = "tile128x64", 128, 64
    else:
        form, bm, bn = "tile64", 64, 64
    return form if cdiv(out, bm) * slots(tokens, groups, bn) <= LIM else "not_taken"


def grouped_form(pkg, tokens, groups, out, inf, cus):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_linear24_grouped_form(tokens, groups, out, inf, cus, ctypes.byref(f)) == 0
    assert pkg.linear24_grouped_form(tokens, groups, out, inf, cus=cus) == FORMS[f.value]
    return FORMS[f.value]


def test_form_query_is_the_stated_rule(pkg):
    assert pkg.lib().sm_linear24_grouped_form(8, 2, 8, 64, 256, None) == INVALID and b"sm_linear24_grouped_form" in _err(pkg)
    seen = set()

    def same(tokens, groups, out, inf, cus):
        got = grouped_form(pkg, tokens, groups, out, inf, cus)
        assert got == rule(tokens, groups, out, inf, cus), (tokens, groups, out, inf, cus)
        seen.add(got)
        return got

    for tokens, groups, out, inf, cus in itertools.product((0, 1, 16, 17, 64, 65, 128, 129, 512, 2048, 8192), (0, 1, 2, 3, 8, 64, MAXG, MAXG + 1),
                                                           (0, 1, 65, 4096, 8193, 11000, 28672, 1 << 20), (64, 96, 4096), (1, 128, 256, 304)):
        same(tokens, groups, out, inf, cus)
    assert seen == set(FORMS) - {"decode"}
    # the mean: ceil(tokens / groups) 64 / 65 decides the 128-token tile
    assert same(65 * 3, 3, 128 * 256, 64, 256) == "tile128" and same(64 * 3, 3, 128 * 256, 64, 256) == "tile128x64"
    assert same(64 * 3 + 1, 3, 128 * 256, 64, 256) == "tile128" and same(16, 1, 8192, 64, 256) == "tile64"     # (never decode)
    assert same(300, 3, 11000, 64, 256) == "tile128"                                                            # 86 * 3 = 258 workgroups
    # the cus boundary of each tile, at 256
    assert same(256, 2, 128 * 128, 64, 256) == "tile128" and same(256, 2, 128 * 127, 64, 256) == "tile128x64"
    assert same(256, 2, 128 * 127 + 1, 64, 256) == "tile128"
    assert same(128, 2, 128 * 128, 64, 256) == "tile128x64" and same(128, 2, 128 * 127, 64, 256) == "tile64"
    assert same(64, 2, 128 * 256, 64, 256) == "tile128x64" and same(64, 2, 128 * 255, 64, 256) == "tile64"
    # the group limit and groups * out
    assert same(8192, MAXG, 64, 64, 256) != "not_taken" and same(8192, MAXG + 1, 64, 64, 256) == "not_taken"
    assert same(8, 2, LIM // 2, 64, 256) != "not_taken" and same(8, 2, LIM // 2 + 1, 64, 256) == "not_taken"
    assert same(8, 1, LIM, 64, 256) != "not_taken" and same(8, 1, BIG, 64, 256) == "not_taken" and same(0, 2, LIM // 2 + 1, 64, 256) == "not_taken"
    assert grouped_form(pkg, 8, 1 << 62, 4, 64, 256) == "not_taken"
    # the grid limit is read on tiles_m * slots: 2^16 tile rows x (2^15 - 1 token tiles + groups - 1 slots)
    out = 128 << 16
    t = (128 << 15) - 128
    assert same(t, 1, out, 64, 256) == "tile128" and same(t, 2, out, 64, 256) == "not_taken" and same(t - 128, 2, out, 64, 256) == "tile128"
    assert cdiv(out, 128) * slots(t, 1, 128) <= LIM < cdiv(out, 128) * slots(t, 2, 128)
    # cus = 0 asks the device (256 when none is visible): a valid answer either way
    assert grouped_form(pkg, 300, 3, 8196, 192, 0) in FORMS[3:]


def library_slots(pkg, tokens, groups):
    """The slot count the LIBRARY sizes a 128 x 128 grid with, read off the form query's grid limit: the largest tile-row count M with
    M * slots <= 2^31 - 1 is where TILE128 turns into NOT_TAKEN, and for M >= 2^16 only one integer `slots` has that M."""
    lo, hi = 1, LIM // (128 * groups)                  # tile rows: groups * out stays a 31-bit count
    taken = lambda m: grouped_form(pkg, tokens, groups, 128 * m, 64, 256) == "tile128"
    assert taken(lo) and not taken(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if taken(mid) else (lo, mid)
    assert lo >= 1 << 16
    s_max, s_min = LIM // lo, LIM // (lo + 1) + 1      # lo * s <= LIM < (lo + 1) * s
    assert s_max == s_min
    return s_max


def test_the_library_sizes_its_grid_with_the_slot_bound(pkg):
    """linear24_grouped_slots itself, through sm_linear24_grouped_form: equal to the formula, hence (next test) a bound on every routing."""
    rng = np.random.default_rng(6)
    for _ in range(40):
        groups = int(rng.integers(1, 9))
        tokens = int(rng.integers(1 << 18, 1 << 21))
        assert library_slots(pkg, tokens, groups) == slots(tokens, groups, 128), (tokens, groups)
    assert library_slots(pkg, 1 << 20, 1) == 1 << 13 and library_slots(pkg, (1 << 20) + 1, 8) == (1 << 13) + 8


def test_slot_bound_covers_every_distribution(pkg):
    """slots = min(tokens, ceil(tokens / BN) + groups - 1) >= sum_g ceil(c_g / BN) for every composition of at most `tokens` tokens.
    This proves the FORMULA restated above, not the library's code: test_the_library_sizes_its_grid_with_the_slot_bound ties the two."""
    for bn in (2, 3):
        for groups in range(1, 5):
            for tokens in range(0, 13):
                worst = 0
                for c in itertools.product(range(tokens + 1), repeat=groups):
                    if sum(c) <= tokens:
                        worst = max(worst, sum(cdiv(x, bn) for x in c))
                assert worst <= slots(tokens, groups, bn), (bn, groups, tokens)
                if groups == 1 or tokens <= groups:     # one group, or one token per group: the bound is attained
                    assert worst == slots(tokens, groups, bn), (bn, groups, tokens)
    rng = np.random.default_rng(5)
    for bn in (64, 128):
        for _ in range(2000):
            groups = int(rng.integers(1, 65))
            tokens = int(rng.integers(0, 5000))
            cuts = np.sort(rng.integers(0, tokens + 1, groups + 1))
            c = np.diff(cuts)
            assert int(np.sum(-(-c // bn))) <= slots(tokens, groups, bn)


def test_python_wrappers_refuse_wrong_dtypes(pkg):
    torch = pytest.importorskip("torch")
    x8 = torch.zeros(64, dtype=torch.uint8).view(torch.float8_e4m3fn)
    h, b, f = torch.zeros(64, dtype=torch.float16), torch.zeros(64, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.float32)
    i32, i64 = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    blob = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(pkg.SparsifymeError, match="both float16 or both bfloat16"):
        pkg.linear24_grouped(blob, h, b, i32, 2, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="group_offsets is int32"):
        pkg.linear24_grouped(blob, h, h, i64, 2, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="group_offsets is int32"):
        pkg.linear24_grouped_glu(blob, h, h, i64, 2, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="act is one of"):
        pkg.linear24_grouped_glu(blob, h, h, i32, 2, 1, 1, 64, act="gelu")
    with pytest.raises(pkg.SparsifymeError, match="bias is float32"):
        pkg.linear24_grouped_glu(blob, h, h, i32, 2, 1, 1, 64, bias=h)
    with pytest.raises(pkg.SparsifymeError, match="float8"):
        pkg.linear24_grouped_fp8(blob, h, h, i32, 2, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="group_offsets is int32"):
        pkg.linear24_grouped_fp8(blob, x8, h, f, 2, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="w_scale is float32"):
        pkg.linear24_grouped_fp8(blob, x8, h, i32, 2, 1, 1, 64, w_scale=h)
    with pytest.raises(pkg.SparsifymeError, match="group_offsets is int32"):
        pkg.linear24_grouped_glu_fp8(blob, x8, h, i64, 2, 1, 1, 64)
    with pytest.raises(pkg.SparsifymeError, match="x_scale is float32"):
        pkg.linear24_grouped_glu_fp8(blob, x8, h, i32, 2, 1, 1, 64, x_scale=h)
