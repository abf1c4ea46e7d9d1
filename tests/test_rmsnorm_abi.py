"""sm_rmsnorm_{f16,bf16} and sm_rmsnorm_form without a GPU: the three symbols are declared, exported and bound with the header's arity and
prototype, the #defines match the Python constants; every status is returned before any device work (fake pointers, never dereferenced),
in the order the header states and with a text that names the entry point and the limit; the zero-extent successes sit behind those
checks; sm_rmsnorm_form at 0, 8, both sides of SM_RMSNORM_LANES_MAX_HIDDEN and of SM_RMSNORM_MAX_HIDDEN and at hidden % 8 != 0; and the
numpy restatement of the definition the GPU test uses (tests/rmsnorm_testlib.py): fp32 to the operation against fp64 within the bound in
both summation orders, against the torch spelling on the CPU, and bit-identical in both orders on the integer class."""
import ctypes
import os
import re

import numpy as np
import pytest

import rmsnorm_testlib as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
MAXH = 16384
WHO = b"sm_rmsnorm_{f16,bf16}"
NAMES = ["sm_rmsnorm_f16", "sm_rmsnorm_bf16"]
# stand-ins for device pointers, all 16-byte aligned and distinct
H, D, G, R, N, Q, S = (ctypes.c_void_p(0x10000 * (i + 1)) for i in range(7))


def _err(pkg):
    return pkg.lib().sm_last_error()


def call(pkg, name="sm_rmsnorm_bf16", h=H, d=D, g=G, res=R, n=N, q=Q, rs=S, tokens=4, hidden=64, ldh=None, ldd=None, ldn=None, ldq=None, eps=1e-6, fmt=0):
    ld = lambda v: hidden if v is None else v
    return getattr(pkg.lib(), name)(h, d, g, res, n, q, rs, tokens, hidden, ld(ldh), ld(ldd), ld(ldn), ld(ldq), eps, fmt, None)


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES + ["sm_rmsnorm_form"]:
        assert name + "(" in header and name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    sz, ci, cf, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    for name in NAMES:
        assert pkg._SIGS[name] == [vp] * 7 + [sz] * 6 + [cf, ci, vp], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(proto.split(",")) == 16 == len(pkg._SIGS[name])
        assert re.search(r"const void\* H,\s*const void\* D,\s*const void\* gamma,\s*void\* res_out,\s*void\* N,\s*void\* Q,\s*float\* row_scale,\s*size_t tokens,"
                         r"\s*size_t hidden,\s*size_t ldh,\s*size_t ldd,\s*size_t ldn,\s*size_t ldq,\s*float eps,\s*int fmt,\s*sm_stream_t stream", proto), name
    assert pkg._SIGS["sm_rmsnorm_form"][0] == sz and len(pkg._SIGS["sm_rmsnorm_form"]) == 2
    assert re.search(r"int sm_rmsnorm_form\(size_t hidden,\s*int\* form\);", header)
    for k, v in (("SM_RMSNORM_FORM_INVALID", 0), ("SM_RMSNORM_FORM_EMPTY", 1), ("SM_RMSNORM_FORM_LANES", 2), ("SM_RMSNORM_FORM_BLOCK", 3),
                 ("SM_RMSNORM_MAX_HIDDEN", MAXH), ("SM_RMSNORM_LANES_MAX_HIDDEN", pkg.RMSNORM_LANES_MAX_HIDDEN), ("SM_FP8_E4M3", 0), ("SM_FP8_E5M2", 1)):
        assert re.search(r"#define %s %d\b" % (k, v), header), k
    assert pkg.RMSNORM_FORMS == ("invalid", "empty", "lanes", "block") and pkg.RMSNORM_MAX_HIDDEN == MAXH
    # the threshold stays inside the quantiser's register budget, on a multiple of 8
    assert 8 <= pkg.RMSNORM_LANES_MAX_HIDDEN <= 4608 and pkg.RMSNORM_LANES_MAX_HIDDEN % 8 == 0
    assert (rl.FP8["e4m3"], rl.FP8["e5m2"]) == (pkg.FP8_E4M3, pkg.FP8_E5M2)
    assert callable(pkg.rmsnorm) and callable(pkg.rmsnorm_form)
    # the header states the definition to the letter and says what is not covered
    for text in ("h_j = rne16(fp32(H_j) + fp32(D_j))", "S = sum_j fp32(h_j)^2", "ms = S / fp32(hidden)", "r = 1 / sqrtf(ms + eps)",
                 "n_j = rne16((fp32(h_j) * r) * fp32(gamma_j))", "LayerNorm", "1 + gamma", "fp32 gamma", "fp32 activations", "hidden > 16384", "2:4 compress"):
        assert text in header, text


@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_device_work_in_the_stated_order(pkg, name):
    c = lambda **kw: call(pkg, name, **kw)
    P2 = ctypes.c_void_p(0x70008)          # 8-byte aligned only
    # 1. invalid values
    for kw in (dict(h=None), dict(n=None, q=None, rs=None), dict(q=None), dict(rs=None), dict(fmt=2), dict(fmt=-1), dict(ldh=56), dict(ldd=63), dict(ldn=8),
               dict(ldq=63), dict(eps=-1e-6), dict(eps=float("nan")), dict(eps=-float("inf")),
               dict(n=H), dict(res=D), dict(res=N), dict(n=H, res=H, ldn=72), dict(n=D, ldn=72), dict(res=H, d=H)):
        assert c(**kw) == INVALID, kw
        assert WHO + b": invalid argument" in _err(pkg), kw
    # ... what is not read is not checked: ldd without D, ldn without N, ldq and fmt without Q
    for kw in (dict(d=None, ldd=0), dict(n=None, ldn=0), dict(q=None, rs=None, ldq=0, fmt=9), dict(g=None), dict(res=None), dict(eps=0.0), dict(eps=float("inf"))):
        assert c(tokens=0, **kw) == 0, kw
    # ... the allowed aliasings are not refused
    for kw in (dict(res=H), dict(n=D), dict(n=H, res=None), dict(n=H, res=H), dict(d=H, res=None)):
        assert c(tokens=0, **kw) == 0, kw
    # ... and invalid is answered before every not-supported shape
    assert c(h=None, tokens=BIG) == INVALID and c(q=None, hidden=MAXH + 8) == INVALID and c(eps=-1.0, hidden=12, ldh=12, ldd=12, ldn=12, ldq=12) == INVALID
    assert c(res=D, h=P2) == INVALID and c(ldh=BIG - 8, hidden=BIG) == INVALID
    # 2. a dimension or a pitch past 2^31 - 1 ...
    for kw in (dict(tokens=BIG), dict(tokens=1 << 40), dict(ldh=BIG), dict(ldd=BIG), dict(ldn=BIG), dict(ldq=BIG), dict(hidden=BIG, ldh=BIG, ldd=BIG, ldn=BIG, ldq=BIG)):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"2^31-1" in _err(pkg), kw
    # ... before the hidden limit, before hidden % 8, before the alignment
    assert c(tokens=BIG, hidden=MAXH + 8) == NOT_SUPPORTED and b"2^31-1" in _err(pkg)
    for hid in (MAXH + 8, MAXH + 1, 1 << 20):
        assert c(hidden=hid, h=P2) == NOT_SUPPORTED and WHO in _err(pkg) and b"SM_RMSNORM_MAX_HIDDEN" in _err(pkg) and b"16384" in _err(pkg), hid
    for hid in (1, 7, 12, 4097, MAXH - 4):
        assert c(hidden=hid, h=P2) == NOT_SUPPORTED and WHO in _err(pkg) and b"hidden % 8" in _err(pkg), hid
    for kw in (dict(h=P2), dict(d=P2), dict(g=P2), dict(res=P2), dict(n=P2), dict(ldh=68), dict(ldd=68), dict(ldn=76)):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"16-byte aligned" in _err(pkg), kw
    # ... Q and row_scale carry no alignment rule, and a pitch nobody reads none either
    assert c(tokens=0, q=ctypes.c_void_p(0x70003), ldq=67, rs=ctypes.c_void_p(0x80004)) == 0 and c(tokens=0, d=None, ldd=3) == 0
    # 3. a zero extent: success, nothing enqueued (the fake pointers never reach a launch) -- but only behind the checks above
    for kw in (dict(tokens=0), dict(hidden=0), dict(tokens=0, hidden=0), dict(tokens=0, hidden=MAXH), dict(tokens=0, n=None), dict(hidden=0, q=None, rs=None)):
        assert c(**kw) == 0, kw
    assert c(tokens=0, h=None) == INVALID and c(tokens=0, fmt=5) == INVALID and c(hidden=0, eps=-1.0) == INVALID
    assert c(tokens=0, hidden=MAXH + 8) == NOT_SUPPORTED and c(tokens=0, hidden=12) == NOT_SUPPORTED and c(tokens=0, h=P2) == NOT_SUPPORTED
    assert c(hidden=0, tokens=BIG) == NOT_SUPPORTED


def test_form_at_every_boundary(pkg):
    assert pkg.lib().sm_rmsnorm_form(64, None) == INVALID and b"sm_rmsnorm_form" in _err(pkg)
    T = pkg.RMSNORM_LANES_MAX_HIDDEN

    def form(hidden):
        f = ctypes.c_int(-1)
        assert pkg.lib().sm_rmsnorm_form(hidden, ctypes.byref(f)) == 0
        assert pkg.rmsnorm_form(hidden) == pkg.RMSNORM_FORMS[f.value]
        return pkg.RMSNORM_FORMS[f.value]

    assert form(0) == "empty" and form(8) == "lanes" and form(T) == "lanes" and form(T + 8) == "block"
    assert form(MAXH) == "block" and form(MAXH + 8) == "invalid" and form(MAXH + 1) == "invalid" and form(1 << 40) == "invalid"
    for hidden in (1, 4, 7, 9, 12, T - 1, T + 1, T + 4, MAXH - 1):
        assert form(hidden) == "invalid", hidden
    seen = set()
    for hidden in range(0, MAXH + 64, 8):
        want = "empty" if hidden == 0 else "invalid" if hidden > MAXH else "lanes" if hidden <= T else "block"
        assert form(hidden) == want, hidden
        seen.add(want)
    assert seen == set(pkg.RMSNORM_FORMS)


# ------------------------------------------------------------------------------------------------ the numpy restatement
def general_rows(rng, tokens, hidden, ty, sigma):
    H = rl.bits_of(rng.normal(0.0, sigma, (tokens, hidden)), ty)
    D = rl.bits_of(rng.normal(0.0, sigma, (tokens, hidden)), ty)
    g = rl.bits_of(rng.normal(1.0, 0.3, hidden), ty)
    return H, D, g


@pytest.mark.parametrize("ty", rl.TYPES)
@pytest.mark.parametrize("hidden", [8, 72, 520, 4096, 8192])
def test_restatement_in_fp32_against_fp64_and_torch(ty, hidden):
    import torch
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    rng = np.random.default_rng(700 + hidden)
    worst = 0.0
    for sigma in (0.01, 1.0, 30.0):
        H, D, g = general_rows(rng, 6, hidden, ty, sigma)
        h = rl.add_round(H, D, ty)
        # the add: one fp32 add, one rounding -- the torch spelling's bits
        tH, tD = (torch.from_numpy(x.view(np.int16)).view(tdt) for x in (H, D))
        assert np.array_equal((tH.float() + tD.float()).to(tdt).view(torch.int16).numpy().view(np.uint16), h)
        for eps in (1e-6, 1e-5):
            for order in ("seq", "tree"):
                n = rl.norm32(h, g, eps, ty, order)
                ratio = rl.worst_ratio(n, h, g, eps, ty)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (sigma, eps, order, ratio)
            # the torch spelling on the CPU: add, fp32 pow / mean / rsqrt / mul / mul, cast (its rsqrt and its order differ by a few ulp of fp32)
            th = torch.from_numpy(h.view(np.int16)).view(tdt).float()
            tn = (th * torch.rsqrt(th.pow(2).mean(-1, keepdim=True) + eps) * torch.from_numpy(g.view(np.int16)).view(tdt).float()).to(tdt)
            got = rl.f32_of(rl.norm32(h, g, eps, ty), ty).astype(np.float64)
            diff = np.abs(got - tn.double().numpy())
            assert np.all(diff <= rl.ulp16(got, ty)), "more than one ulp of the output type from the torch spelling"
        # without gamma: one multiply
        assert rl.worst_ratio(rl.norm32(h, None, 1e-6, ty), h, None, 1e-6, ty) <= 1.0
    print(f"restatement {ty} hidden {hidden}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("ty", rl.TYPES)
@pytest.mark.parametrize("hidden", [8, 72, 4096, 16384])
def test_integer_class_premise_and_order_independence(ty, hidden):
    rng = np.random.default_rng(900 + hidden)
    H, D, g = rl.integer_rows(rng, 9, hidden, ty)
    h = rl.add_round(H, D, ty)
    assert rl.integer_class(h, g, ty)
    x = rl.f32_of(h, ty)
    assert np.isinf(x).any() and np.isnan(x).any() and (x == 0).all(axis=1).any()
    for eps in (0.0, 1e-6, 0.5):
        a, b = rl.norm32(h, g, eps, ty, "seq"), rl.norm32(h, g, eps, ty, "tree")
        assert rl.same_bits_nan_as_nan(a, b, ty), eps
        n = rl.f32_of(a, ty)
        # an inf in a row: r = 0, zeros and NaN at the inf; an all-zero row: NaN with eps = 0, zeros otherwise
        inf_rows = np.isinf(x).any(axis=1) & ~np.isnan(x).any(axis=1)
        assert np.all(np.isnan(n[inf_rows]) == np.isinf(x[inf_rows])) and np.all(n[inf_rows][~np.isinf(x[inf_rows])] == 0)
        zero_rows = (x == 0).all(axis=1)
        assert np.all(np.isnan(n[zero_rows])) if eps == 0.0 else np.all(n[zero_rows] == 0)
    # the premise is a premise: it refuses what breaks it
    bad = h.copy()
    bad[0, 0] = rl.bits_of(16.0, ty)
    assert not rl.integer_class(bad, g, ty) and not rl.integer_class(h, rl.bits_of(np.full(hidden, 0.5), ty), ty)
