"""MoE routing, the gathered grouped layers and the combine step (sm_moe_route*, sm_linear24_grouped_*gather_*, sm_moe_combine_*) without a
GPU: every new symbol is declared, exported and bound with the right arity; every status is returned before any device work (fake
pointers, never dereferenced) with a text that names the entry point; sm_moe_route_form at both sides of the SINGLE / MULTI threshold
and the workspace size as the header states it; sm_moe_combine_form at both sides of every alignment condition; and the two numpy
references the GPU tests use -- the route against np.argsort(kind="stable"), the combine against an fp64 evaluation on integer data."""
import ctypes
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
MAXG = 1024
SINGLE_MAX, CHUNK = 4096, 4096
E4M3, BF16, SILU = 0, 2, 2
GATHER = [g + "gather_" + s for g in ("sm_linear24_grouped_", "sm_linear24_grouped_glu_") for s in ("f16", "bf16", "fp8")]
ROUTE = ["sm_moe_route", "sm_moe_route_form", "sm_moe_route_workspace_size"]
COMBINE = ["sm_moe_combine_f16", "sm_moe_combine_bf16", "sm_moe_combine_form"]


def _err(pkg):
    return pkg.lib().sm_last_error()


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in GATHER + ROUTE + COMBINE:
        assert name + "(" in header and name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    sz, ci, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    for name in GATHER:   # the twin's signature with (x_index, x_rows) directly after group_offsets
        twin = pkg._SIGS[name.replace("gather_", "")]
        assert pkg._SIGS[name] == twin[:4] + [vp, sz] + twin[4:], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert re.search(r"const int\* group_offsets,\s*const int\* x_index,\s*size_t x_rows,\s*size_t groups,", proto), name
        assert len(proto.split(",")) == len(pkg._SIGS[name])
    assert pkg._SIGS["sm_moe_route"] == [vp, sz, sz, sz, vp, vp, vp, vp, vp, sz, vp]
    assert pkg._SIGS["sm_moe_route_form"][:3] == [sz] * 3 and len(pkg._SIGS["sm_moe_route_form"]) == 4
    assert pkg._SIGS["sm_moe_route_workspace_size"][:3] == [sz] * 3 and len(pkg._SIGS["sm_moe_route_workspace_size"]) == 4
    for name in COMBINE[:2]:
        assert pkg._SIGS[name] == [vp] * 5 + [sz] * 6 + [vp]
    assert pkg._SIGS["sm_moe_combine_form"][:6] == [vp] * 3 + [sz] * 3 and len(pkg._SIGS["sm_moe_combine_form"]) == 7
    for name, proto_n in (("sm_moe_route", 11), ("sm_moe_combine_f16", 12), ("sm_moe_combine_form", 7), ("sm_moe_route_form", 4)):
        assert len(re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1).split(",")) == proto_n == len(pkg._SIGS[name])
    for k, v in (("SM_MOE_ROUTE_FORM_INVALID", 0), ("SM_MOE_ROUTE_FORM_EMPTY", 1), ("SM_MOE_ROUTE_FORM_SINGLE", 2), ("SM_MOE_ROUTE_FORM_MULTI", 3),
                 ("SM_MOE_ROUTE_SINGLE_MAX_PAIRS", SINGLE_MAX), ("SM_MOE_ROUTE_CHUNK", CHUNK), ("SM_MOE_COMBINE_FORM_INVALID", 0),
                 ("SM_MOE_COMBINE_FORM_EMPTY", 1), ("SM_MOE_COMBINE_FORM_SCALAR", 2), ("SM_MOE_COMBINE_FORM_VEC", 3)):
        assert re.search(r"#define %s %d\b" % (k, v), header), k
    assert pkg.MOE_ROUTE_FORMS == ("invalid", "empty", "single", "multi") and pkg.MOE_COMBINE_FORMS == ("invalid", "empty", "scalar", "vec")
    assert pkg.MOE_ROUTE_SINGLE_MAX_PAIRS == SINGLE_MAX and pkg.MOE_ROUTE_CHUNK == CHUNK
    for fn in ("moe_route", "moe_route_form", "moe_route_workspace_size", "moe_combine", "moe_combine_form"):
        assert callable(getattr(pkg, fn))


# ------------------------------------------------------------------------------------------------ sm_moe_route
def route(pkg, ids=P, tokens=8, top_k=2, groups=4, off=P, st=P, sp=P, pp=P, ws=None, nb=0):
    return pkg.lib().sm_moe_route(ids, tokens, top_k, groups, off, st, sp, pp, ws, nb, None)


def ws_size(pkg, tokens, top_k, groups):
    n = ctypes.c_size_t(12345)
    rc = pkg.lib().sm_moe_route_workspace_size(tokens, top_k, groups, ctypes.byref(n))
    return rc, n.value


def route_form(pkg, tokens, top_k, groups):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_moe_route_form(tokens, top_k, groups, ctypes.byref(f)) == 0
    assert pkg.moe_route_form(tokens, top_k, groups) == pkg.MOE_ROUTE_FORMS[f.value]
    return pkg.MOE_ROUTE_FORMS[f.value]


def test_route_statuses_before_any_device_work(pkg):
    multi = dict(tokens=SINGLE_MAX + 1, top_k=1)
    need = ws_size(pkg, SINGLE_MAX + 1, 1, 4)[1]
    assert need == 2 * 4 * 4
    for kw in (dict(ids=None), dict(off=None), dict(st=None), dict(sp=None), dict(pp=None), dict(multi), dict(ws=P, nb=need - 1, **multi),
               dict(ws=None, nb=need, **multi)):
        assert route(pkg, **kw) == INVALID, kw
        assert b"sm_moe_route: invalid argument" in _err(pkg), kw
    # ... answered before the not-supported shapes
    assert route(pkg, ids=None, groups=MAXG + 1) == INVALID and route(pkg, pp=None, tokens=BIG) == INVALID
    for kw in (dict(tokens=BIG, top_k=1), dict(tokens=1 << 16, top_k=1 << 15), dict(tokens=1 << 40, top_k=1 << 40), dict(groups=MAXG + 1),
               dict(groups=1 << 50)):
        assert route(pkg, **kw) == NOT_SUPPORTED, kw
        assert b"sm_moe_route" in _err(pkg) and b"2^31-1" in _err(pkg) and b"SM_LINEAR24_MAX_GROUPS" in _err(pkg), kw
    # groups == 0: success, nothing enqueued (the fake pointers are never handed to a launch); the workspace may then be NULL
    assert route(pkg, groups=0) == 0 and route(pkg, groups=0, tokens=1 << 20, top_k=8) == 0 and route(pkg, groups=0, tokens=0) == 0
    assert route(pkg, groups=0, ids=None) == INVALID


def test_route_form_and_workspace_size_as_the_header_states_them(pkg):
    assert pkg.lib().sm_moe_route_form(8, 2, 4, None) == INVALID and b"sm_moe_route_form" in _err(pkg)
    assert pkg.lib().sm_moe_route_workspace_size(8, 2, 4, None) == INVALID and b"sm_moe_route_workspace_size" in _err(pkg)

    def rule(tokens, top_k, groups):
        Pn = tokens * top_k
        if Pn > LIM or groups > MAXG:
            return "invalid", None
        if Pn == 0 or groups == 0:
            return "empty", 0
        return ("single", 0) if Pn <= SINGLE_MAX else ("multi", -(-Pn // CHUNK) * groups * 4)

    seen = set()
    for tokens in (0, 1, 16, 511, 512, 513, 2048, 4096, 4097, 8192, 1 << 20, LIM, BIG):
        for top_k in (0, 1, 2, 8):
            for groups in (0, 1, 8, 256, MAXG, MAXG + 1):
                form, size = rule(tokens, top_k, groups)
                assert route_form(pkg, tokens, top_k, groups) == form, (tokens, top_k, groups)
                rc, n = ws_size(pkg, tokens, top_k, groups)
                assert (rc, n) == ((NOT_SUPPORTED, 12345) if size is None else (0, size)), (tokens, top_k, groups)
                seen.add(form)
    assert seen == {"invalid", "empty", "single", "multi"}
    # both sides of the one SINGLE / MULTI threshold: P = tokens * top_k against SM_MOE_ROUTE_SINGLE_MAX_PAIRS, whatever the group count
    for groups in (1, 8, MAXG):
        assert route_form(pkg, SINGLE_MAX, 1, groups) == "single" and route_form(pkg, SINGLE_MAX + 1, 1, groups) == "multi"
        assert route_form(pkg, SINGLE_MAX // 8, 8, groups) == "single" and route_form(pkg, SINGLE_MAX // 8 + 1, 8, groups) == "multi"
        assert ws_size(pkg, SINGLE_MAX, 1, groups) == (0, 0) and ws_size(pkg, SINGLE_MAX + 1, 1, groups) == (0, 2 * groups * 4)
    # the chunk boundary of the size, and the limits
    assert ws_size(pkg, 2 * CHUNK, 1, 8)[1] == 2 * 8 * 4 and ws_size(pkg, 2 * CHUNK + 1, 1, 8)[1] == 3 * 8 * 4
    assert route_form(pkg, LIM, 1, MAXG) == "multi" and route_form(pkg, BIG, 1, 1) == "invalid" and route_form(pkg, 1 << 62, 1 << 62, 1) == "invalid"
    assert ws_size(pkg, LIM, 1, MAXG)[1] == -(-LIM // CHUNK) * MAXG * 4


# ------------------------------------------------------------------------------------------------ the gathered layers
def g_p16(pkg, name, blob=P, X=P, Y=P, off=P, xi=P, xr=8, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, ep=None, act=None):
    return getattr(pkg.lib(), name)(blob, X, Y, off, xi, xr, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, 1.0, 0.0, ep,
                                    None)


def g_p8(pkg, name, blob=P, X=P, Y=P, off=P, xi=P, xr=8, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, ep=None, act=None):
    return getattr(pkg.lib(), name)(blob, X, Y, off, xi, xr, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, E4M3, E4M3,
                                    BF16, 1.0, 0.0, None, None, ep, None)


def g_g16(pkg, name, blob=P, X=P, Y=P, off=P, xi=P, xr=8, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, ep=None, act=SILU):
    return getattr(pkg.lib(), name)(blob, X, Y, off, xi, xr, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, act, None, None)


def g_g8(pkg, name, blob=P, X=P, Y=P, off=P, xi=P, xr=8, groups=2, tokens=8, out=8, inf=64, ldx=None, ldy=None, ep=None, act=SILU):
    return getattr(pkg.lib(), name)(blob, X, Y, off, xi, xr, groups, tokens, out, inf, inf if ldx is None else ldx, out if ldy is None else ldy, E4M3, E4M3,
                                    BF16, act, None, None, None, None)


GATHER_CALLS = [("sm_linear24_grouped_gather_f16", g_p16, b"sm_linear24_grouped_gather_{f16,bf16}", False),
                ("sm_linear24_grouped_gather_bf16", g_p16, b"sm_linear24_grouped_gather_{f16,bf16}", False),
                ("sm_linear24_grouped_gather_fp8", g_p8, b"sm_linear24_grouped_gather_fp8", False),
                ("sm_linear24_grouped_glu_gather_f16", g_g16, b"sm_linear24_grouped_glu_gather_{f16,bf16}", True),
                ("sm_linear24_grouped_glu_gather_bf16", g_g16, b"sm_linear24_grouped_glu_gather_{f16,bf16}", True),
                ("sm_linear24_grouped_glu_gather_fp8", g_g8, b"sm_linear24_grouped_glu_gather_fp8", True)]


class Epi(ctypes.Structure):   # sm_epilogue_t
    _fields_ = [("bias", ctypes.c_void_p), ("bias_dim", ctypes.c_int), ("act", ctypes.c_int), ("act_arg", ctypes.c_float), ("R", ctypes.c_void_p),
                ("strideR", ctypes.c_size_t)]


@pytest.mark.parametrize("name,fn,who,gated", GATHER_CALLS, ids=[c[0] for c in GATHER_CALLS])
def test_gather_statuses_are_the_twins_with_the_two_additions(pkg, name, fn, who, gated):
    call = lambda **kw: fn(pkg, name, **kw)
    # 1. the epilogue / the activation first, also in front of a null x_index
    if gated:
        assert call(act=3, xi=None) == INVALID and who in _err(pkg) and b"act is not SM_GLU_ACT_*" in _err(pkg)
    else:
        bad = Epi(None, 5, 0, 0.0, None, 0)
        assert call(ep=ctypes.byref(bad), xi=None) == INVALID and who + b": invalid epilogue" in _err(pkg)
    # 2. the first invalid-value test, with the two additions
    for kw in (dict(xi=None), dict(xr=0), dict(blob=None), dict(X=None), dict(Y=None), dict(off=None), dict(blob=ODD), dict(ldx=63), dict(ldy=7)):
        assert call(**kw) == INVALID, kw
        assert who + b": invalid argument" in _err(pkg) and b"null x_index, x_rows == 0" in _err(pkg) and b"null group_offsets" in _err(pkg), kw
    # ... before the dimension test, where x_rows >= 2^31 belongs
    assert call(xi=None, tokens=BIG) == INVALID and call(xr=0, xi=P, inf=96, ldx=96) == INVALID
    for kw in (dict(xr=BIG), dict(xr=1 << 40), dict(tokens=BIG)):
        assert call(**kw) == NOT_SUPPORTED, kw
        assert who in _err(pkg) and b"dimension exceeds 2^31-1" in _err(pkg), kw
    assert call(xr=LIM, tokens=0) == 0
    # ... before the group limit, in_features % 64 and the alignment of X
    assert call(xr=BIG, groups=MAXG + 1) == NOT_SUPPORTED and b"dimension exceeds" in _err(pkg)
    assert call(groups=MAXG + 1, inf=96, ldx=96) == NOT_SUPPORTED and b"SM_LINEAR24_MAX_GROUPS" in _err(pkg)
    assert call(xr=BIG, inf=96, ldx=96) == NOT_SUPPORTED and b"dimension exceeds" in _err(pkg)
    assert call(inf=96, ldx=96) == NOT_SUPPORTED and b"in_features" in _err(pkg)
    assert call(X=ODD) == NOT_SUPPORTED and b"16-byte aligned rows of X" in _err(pkg)
    # empty: success, nothing enqueued
    assert call(tokens=0) == 0 and call(out=0, ldy=0) == 0 and call(groups=0) == 0
    assert call(groups=0, xi=None) == INVALID and call(tokens=0, xr=0) == INVALID
    # the grid limit, as the twin
    out = (64 << 16) if gated else (128 << 16)
    assert call(groups=1, tokens=LIM, xr=LIM, out=out, ldy=out) == NOT_SUPPORTED and who + b": grid too large" in _err(pkg)


# ------------------------------------------------------------------------------------------------ sm_moe_combine
def combine(pkg, name="sm_moe_combine_f16", Yp=P, pp=P, w=None, R=None, out=P, tokens=4, top_k=2, hidden=8, rows_p=8, ldp=None, ldo=None):
    return getattr(pkg.lib(), name)(Yp, pp, w, R, out, tokens, top_k, hidden, rows_p, hidden if ldp is None else ldp, hidden if ldo is None else ldo, None)


def combine_form(pkg, Yp=P, R=None, out=P, hidden=64, ldp=64, ldo=64):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_moe_combine_form(Yp, R, out, hidden, ldp, ldo, ctypes.byref(f)) == 0
    as_int = lambda v: None if v is None else v.value
    assert pkg.moe_combine_form(as_int(Yp), as_int(R), as_int(out), hidden, ldp, ldo) == pkg.MOE_COMBINE_FORMS[f.value]
    return pkg.MOE_COMBINE_FORMS[f.value]


@pytest.mark.parametrize("name", COMBINE[:2])
def test_combine_statuses_before_any_device_work(pkg, name):
    who = b"sm_moe_combine_{f16,bf16}"
    for kw in (dict(Yp=None), dict(pp=None), dict(out=None), dict(ldp=7), dict(ldo=7), dict(Yp=None, tokens=BIG)):
        assert combine(pkg, name, **kw) == INVALID, kw
        assert who + b": invalid argument" in _err(pkg), kw
    for kw in (dict(tokens=BIG), dict(top_k=BIG), dict(tokens=1 << 16, top_k=1 << 15), dict(hidden=BIG, ldp=BIG, ldo=BIG), dict(rows_p=BIG), dict(ldp=BIG),
               dict(ldo=BIG)):
        assert combine(pkg, name, **kw) == NOT_SUPPORTED, kw
        assert who in _err(pkg) and b"2^31-1" in _err(pkg), kw
    # a zero extent: success, nothing enqueued (the fake pointers never reach a launch); weights and R may be NULL or not
    for kw in (dict(tokens=0), dict(top_k=0), dict(hidden=0), dict(tokens=0, w=P, R=P), dict(hidden=0, ldp=0, ldo=0)):
        assert combine(pkg, name, **kw) == 0, kw
    assert combine(pkg, name, tokens=0, rows_p=BIG) == NOT_SUPPORTED


def test_combine_form_at_both_sides_of_every_alignment_condition(pkg):
    assert pkg.lib().sm_moe_combine_form(P, None, P, 64, 64, 64, None) == INVALID and b"sm_moe_combine_form" in _err(pkg)
    assert combine_form(pkg) == "vec" and combine_form(pkg, R=P) == "vec"
    assert combine_form(pkg, hidden=56, ldp=56, ldo=56) == "vec" and combine_form(pkg, hidden=8, ldp=8, ldo=8) == "vec"
    for h in (1, 7, 9, 60, 63):                                         # hidden % 8
        assert combine_form(pkg, hidden=h, ldp=64, ldo=64) == "scalar", h
    assert combine_form(pkg, ldp=72) == "vec" and combine_form(pkg, ldp=68) == "scalar" and combine_form(pkg, ldp=65) == "scalar"     # ldp % 8
    assert combine_form(pkg, ldo=72) == "vec" and combine_form(pkg, ldo=68) == "scalar" and combine_form(pkg, ldo=71) == "scalar"     # ldo % 8
    assert combine_form(pkg, Yp=ODD) == "scalar" and combine_form(pkg, out=ODD) == "scalar" and combine_form(pkg, R=ODD) == "scalar"  # 16 bytes
    assert combine_form(pkg, Yp=ctypes.c_void_p(0x1002)) == "scalar" and combine_form(pkg, R=ctypes.c_void_p(0x100e), out=P) == "scalar"
    assert combine_form(pkg, hidden=0) == "empty" and combine_form(pkg, hidden=0, ldp=0, ldo=0) == "empty"
    for kw in (dict(Yp=None), dict(out=None), dict(ldp=63), dict(ldo=63), dict(hidden=BIG, ldp=BIG, ldo=BIG), dict(ldp=BIG), dict(ldo=BIG)):
        assert combine_form(pkg, **kw) == "invalid", kw


# ------------------------------------------------------------------------------------------------ the numpy references
def route_ref(ids, top_k, groups):
    """include/sparsifyme.h, sm_moe_route, to the letter: one pass over the pairs in ascending p"""
    ids = np.asarray(ids, dtype=np.int64)
    Pn = len(ids)
    kept = (ids >= 0) & (ids < groups)
    off = np.zeros(groups + 1, dtype=np.int32)
    for g in range(groups):
        off[g + 1] = off[g] + int(np.sum(ids[kept] == g))
    nxt = off[:-1].astype(np.int64).copy()
    st, sp, pp = (np.full(Pn, -1, dtype=np.int32) for _ in range(3))
    for p in range(Pn):
        if kept[p]:
            s = nxt[ids[p]]
            nxt[ids[p]] += 1
            sp[s], st[s], pp[p] = p, p // top_k, s
    return off, st, sp, pp


def test_route_reference_against_a_stable_argsort():
    rng = np.random.default_rng(11)
    pool = [([], 1, 3), ([0], 1, 1), ([5, -1, 9], 1, 4), ([2, 2, 2, 2], 2, 3)]
    for _ in range(60):
        groups, top_k = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        tokens = int(rng.integers(0, 70))
        lo, hi = (0, groups) if rng.random() < 0.5 else (-3, groups + 4)
        pool.append((rng.integers(lo, hi, tokens * top_k), top_k, groups))
    for ids, top_k, groups in pool:
        ids = np.asarray(ids, dtype=np.int64)
        off, st, sp, pp = route_ref(ids, top_k, groups)
        kept = (ids >= 0) & (ids < groups)
        key = np.where(kept, ids, groups)                                  # dropped pairs sort behind every expert
        order = np.argsort(key, kind="stable")
        V = int(kept.sum())
        assert off[-1] == V and np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(ids[kept], minlength=groups))]))
        assert np.array_equal(sp[:V], order[:V]) and np.all(sp[V:] == -1) and np.all(st[V:] == -1)
        assert np.array_equal(st[:V], order[:V] // top_k)
        inv = np.full(len(ids), -1)
        inv[order[:V]] = np.arange(V)
        assert np.array_equal(pp, inv)


def combine_ref(Yp, pair_pos, weights, R, tokens, top_k, hidden, rows_p):
    """fp32 to the operation: s = R or +0; q = w * y as a float32 multiply, s = s + q as a float32 add, j ascending.  Returns the fp32 sums
    (the caller rounds them once to the output type)."""
    Yp = np.asarray(Yp, dtype=np.float32)
    s = np.zeros((tokens, hidden), dtype=np.float32) if R is None else np.asarray(R, dtype=np.float32)[:, :hidden].copy()
    for t in range(tokens):
        for j in range(top_k):
            pos = int(pair_pos[t * top_k + j])
            if pos < 0 or pos >= rows_p:
                continue
            y = Yp[pos, :hidden]
            q = y if weights is None else (np.float32(weights[t * top_k + j]) * y).astype(np.float32)
            s[t] = (s[t] + q).astype(np.float32)
    return s


def test_combine_reference_against_fp64_on_integer_data():
    """integers small enough that every product and partial sum is exact in fp32 (|w y| <= 8 * 64, sums < 2^24): fp32 == fp64"""
    rng = np.random.default_rng(12)
    for top_k, with_w, with_r in ((1, False, False), (2, True, False), (3, True, True), (8, False, True), (8, True, True)):
        tokens, hidden, rows_p = 9, 13, 40
        Pn = tokens * top_k
        Yp = rng.integers(-64, 65, (rows_p, hidden)).astype(np.float32)
        pos = rng.integers(-3, rows_p + 4, Pn)
        pos[:top_k] = -1                                                  # token 0: every pair dropped
        w = rng.integers(-8, 9, Pn).astype(np.float32) if with_w else None
        R = rng.integers(-100, 101, (tokens, hidden)).astype(np.float32) if with_r else None
        got = combine_ref(Yp, pos, w, R, tokens, top_k, hidden, rows_p)
        want = np.zeros((tokens, hidden)) if R is None else R.astype(np.float64)
        for p in range(Pn):
            if 0 <= pos[p] < rows_p:
                want[p // top_k] += (1.0 if w is None else float(w[p])) * Yp[pos[p]].astype(np.float64)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
        assert np.array_equal(got[0], np.zeros(hidden) if R is None else R[0])
