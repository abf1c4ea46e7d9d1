"""sm_linear24_glu_fp8 on the device: Y[tokens][hidden] = act(g) * u with g, u the two halves of a fused gate/up 2:4 weight, fp8
operands, token-major in and out, one launch.  The reference is this file's own numpy fp64 on its own decode of the fp8 bytes.

1. each half alone (the other held at exactly 1) equals the matching columns of sm_linear24_fp8 on the same blob bit for bit: the row
   map, the clamps and both accumulators of every tile instantiation and of the decode form;
2. fp32 out equals the np.float32 product of the two column halves of sm_linear24_fp8's fp32 output bit for bit (scales, bias);
3. integer operands: the fp64 product rounded once to the output type, bit for bit, every form and type;
4. SiLU alone, 65536 gates over every binade of +-[2^-30, 2^7] and the special values, inside the DERIVED bound
   4 * 2^-24 |silu| + 2^-120 (exp 2^-23 + add 2^-24 + divide 2^-24; the cut to -0);
5. every activation against fp64 with bias and scales, decode and a tile form per output type;
6. NaN / inf reach exactly the outputs they feed; two runs and a hipGraph replay give the same bits.
Every call runs on X with ldx > in and NaN bytes in the padding and behind the last token, and on Y with ldy > hidden whose slack
columns and tail row are guarded by a sentinel.  Every test named for a form asks linear24_glu_form which form its shape runs."""
import functools
import os

import numpy as np
import pytest
import torch
from linear24_testlib import (DEV, INT_SHAPES, NAN_BYTE, ODT, OUTS, PAIRS, ROUND, SENTINEL, SHAPES, SID, TDT, TINY, U_OPS, act64,
                              decode8, dev8, encode8, f32dev, mask24, silu64)

pytestmark = pytest.mark.gpu

IDT = {"f32": torch.int32, "f16": torch.int16, "bf16": torch.int16}
ACTS = ["none", "relu", "silu"]


def compress(pkg, wb, fmt):
    rows, inf = wb.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 1, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24_fp8(dev8(wb, fmt), rows, inf, inf, 1, rows * inf, blob)
    return blob


def bits(t):
    return t.contiguous().view(IDT[{v: k for k, v in ODT.items()}[t.dtype]])


def check_form(pkg, tokens, hidden, inf, want):
    assert pkg.linear24_glu_form(tokens, hidden, inf) == want
    assert pkg.linear24_fp8_form(tokens, 2 * hidden, inf) == want      # the plain layer takes the same blob through the same form


def padded_x(xb, fx):
    """[tokens + 1][in + 16] with NaN bytes in the padding and in the row behind the last token"""
    tokens, inf = xb.shape
    xp = np.full((tokens + 1, inf + 16), NAN_BYTE[fx], dtype=np.uint8)
    xp[:tokens, :inf] = xb
    return dev8(xp, fx), inf + 16


def glu(pkg, blob, xb, fw, fx, o, tokens, hidden, inf, act, ws=None, xs=None, bias=None, Xp=None):
    """The gated call on padded X and a sentinel-guarded Y; returns Y[:tokens, :hidden] (a copy)."""
    if Xp is None:
        Xp = padded_x(xb, fx)
    X, ldx = Xp
    ldy = hidden + 12
    Y = torch.full((tokens + 1, ldy), SENTINEL, dtype=ODT[o], device=DEV)
    pkg.linear24_glu_fp8(blob, X, Y, tokens, hidden, inf, act=act, w_dtype=TDT[fw], w_scale=ws, x_scale=xs, bias=bias, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    assert bool((Y[:tokens, hidden:] == SENTINEL).all()) and bool((Y[tokens] == SENTINEL).all()), "slack columns or the tail row of Y were written"
    return Y[:tokens, :hidden].contiguous()


def plain(pkg, blob, xb, fw, fx, o, tokens, hidden, inf, ws=None, xs=None, bias=None, Xp=None):
    """sm_linear24_fp8 on the same blob: [tokens][2 hidden], alpha 1, beta 0, the bias through SM_BIAS_COL."""
    if Xp is None:
        Xp = padded_x(xb, fx)
    X, ldx = Xp
    Y = torch.full((tokens, 2 * hidden), SENTINEL, dtype=ODT[o], device=DEV)
    pkg.linear24_fp8(blob, X, Y, tokens, 2 * hidden, inf, w_dtype=TDT[fw], ldx=ldx, w_scale=ws, x_scale=xs,
                     epilogue=pkg.Epilogue(bias=bias, bias_dim="col") if bias is not None else None)
    torch.cuda.synchronize()
    return Y


@functools.lru_cache(maxsize=None)
def rand_bytes(shape, fw, fx, seed, wlo=0.0):
    """W[2 hidden][in] 2:4 with the kept values in U(-2, 2) (wlo = 0.25: |w| >= 0.25, no kept value rounds to zero), X in U(-2, 2): fp8 bytes."""
    tokens, hidden, inf = shape
    rng = np.random.default_rng(seed)
    w = rng.uniform(wlo, 2.0, (2 * hidden, inf)) * rng.choice(np.array([-1.0, 1.0]), size=(2 * hidden, inf))
    wb = encode8(np.where(mask24(rng, 2 * hidden, inf), w, 0.0), fw)
    xb = encode8(rng.uniform(-2, 2, (tokens, inf)), fx)
    return wb, xb


# ------------------------------------------------------------------------------------------------ 1. each half against the plain layer
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
@pytest.mark.parametrize("fw,fx", PAIRS)
def test_each_half_equals_the_plain_layer_bit_for_bit(gpu, fw, fx, shape):
    """Up rows = a single 1 at column 0 and X[:, 0] = 1 make u exactly 1: with act NONE Y is g, which must be columns 0 .. hidden-1 of
    sm_linear24_fp8 on the same blob; mirrored with the gate rows held at 1, Y is u = columns hidden .. 2 hidden - 1."""
    pkg = gpu
    tokens, hidden, inf, want = shape
    check_form(pkg, tokens, hidden, inf, want)
    o = OUTS[(SHAPES.index(shape) + PAIRS.index((fw, fx))) % 3]
    wb0, xb0 = rand_bytes(shape[:3], fw, fx, 100 + SHAPES.index(shape))
    xb = xb0.copy()
    xb[:, 0] = encode8(np.ones(1), fx)[0]
    Xp = padded_x(xb, fx)
    one = np.zeros(inf, dtype=np.uint8)
    one[0] = encode8(np.ones(1), fw)[0]
    for half, cols in ((1, slice(0, hidden)), (0, slice(hidden, 2 * hidden))):    # the half held at 1, the columns Y must equal
        wb = wb0.copy()
        wb[half * hidden:(half + 1) * hidden] = one
        blob = compress(pkg, wb, fw)
        got = glu(pkg, blob, xb, fw, fx, o, tokens, hidden, inf, "none", Xp=Xp)
        ref = plain(pkg, blob, xb, fw, fx, o, tokens, hidden, inf, Xp=Xp)
        assert bool((ref[:, half * hidden:(half + 1) * hidden] == 1.0).all())
        bad = torch.nonzero(bits(got) != bits(ref[:, cols]))
        assert bad.numel() == 0, f"{'gate' if half else 'up'} half: first mismatch at (token, feature) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


# ------------------------------------------------------------------------------------------------ 2. fp32 out == the product of the halves
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_fp32_out_is_the_float32_product_of_the_plain_halves(gpu, shape):
    pkg = gpu
    tokens, hidden, inf, want = shape
    check_form(pkg, tokens, hidden, inf, want)
    fw, fx = PAIRS[SHAPES.index(shape) % 4]
    wb, xb = rand_bytes(shape[:3], fw, fx, 200 + SHAPES.index(shape))
    rng = np.random.default_rng(250 + SHAPES.index(shape))
    ws, xs = f32dev(rng.uniform(0.5, 2.0, 2 * hidden)), f32dev(rng.uniform(0.5, 2.0, tokens))
    bias = f32dev(rng.uniform(-2, 2, 2 * hidden))
    blob, Xp = compress(pkg, wb, fw), padded_x(xb, fx)
    P = plain(pkg, blob, xb, fw, fx, "f32", tokens, hidden, inf, ws, xs, bias, Xp).cpu().numpy()
    g, u = P[:, :hidden], P[:, hidden:]
    assert g.dtype == np.float32 and np.isfinite(P).all()
    for act in ("none", "relu"):
        a = g if act == "none" else np.where(g > 0, g, np.float32(0.0))
        ref = torch.from_numpy(np.multiply(a, u, dtype=np.float32))
        got = glu(pkg, blob, xb, fw, fx, "f32", tokens, hidden, inf, act, ws, xs, bias, Xp).cpu()
        bad = torch.nonzero(bits(got) != bits(ref))
        assert bad.numel() == 0, f"{act}: first mismatch at (token, feature) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


# ------------------------------------------------------------------------------------------------ 3. integer-exact
@pytest.mark.parametrize("o", OUTS)
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_operands_give_the_fp64_product_rounded_once(gpu, shape, o):
    """W in {-1, 0, 1} (two kept of four), X integers in [-3, 3], in = 64: |g|, |u| <= 32 * 3 = 96, so g, u and g * u <= 9216 are exact
    in fp32 and finite in fp16; Y is the fp64 product rounded ONCE to the output type (9216 is not exact in bf16 or fp16: the
    rounding is part of the comparison)."""
    pkg = gpu
    tokens, hidden, want = shape
    inf = 64
    check_form(pkg, tokens, hidden, inf, want)
    fw, fx = PAIRS[(INT_SHAPES.index(shape) + OUTS.index(o)) % 4]
    rng = np.random.default_rng(300 + 10 * INT_SHAPES.index(shape) + OUTS.index(o))
    Wn = np.where(mask24(rng, 2 * hidden, inf), rng.choice(np.array([-1.0, 1.0]), size=(2 * hidden, inf)), 0.0)
    Xn = rng.integers(-3, 4, size=(tokens, inf)).astype(np.float64)
    wb, xb = encode8(Wn, fw), encode8(Xn, fx)
    assert np.array_equal(decode8(wb, fw), Wn) and np.array_equal(decode8(xb, fx), Xn)
    acc = Xn @ Wn.T
    g, u = acc[:, :hidden], acc[:, hidden:]
    assert np.abs(acc).max() <= 96
    blob, Xp = compress(pkg, wb, fw), padded_x(xb, fx)
    for act in ("none", "relu"):
        ref = torch.from_numpy((g if act == "none" else np.maximum(g, 0.0)) * u).to(ODT[o])     # integers: fp64 -> fp32 is exact, one rounding follows
        got = glu(pkg, blob, xb, fw, fx, o, tokens, hidden, inf, act, Xp=Xp).cpu()
        bad = torch.nonzero(bits(got) != bits(ref))
        assert bad.numel() == 0, f"{act} -> {o}: first mismatch at {bad[0].tolist()}: got {float(got[tuple(bad[0])])}, want {float(ref[tuple(bad[0])])}"


# ------------------------------------------------------------------------------------------------ margins
MARGINS = {}
TAG = "[fp8]   "


def note_margin(key, ratio, what):
    if key not in MARGINS or ratio > MARGINS[key][0]:
        MARGINS[key] = (ratio, what)


@pytest.fixture(scope="module", autouse=True)
def _margin_report():
    yield
    if not MARGINS:
        return
    lines = [f"{TAG}{key:14s} {r:.4f}  {what}" for key, (r, what) in sorted(MARGINS.items())]
    print("\n".join(["sm_linear24_glu_fp8: worst err / bound"] + lines))
    d = os.environ.get("SM_PARITY_MARGINS_DIR")   # where a run that refreshes profiles/parity_margins_linear24_glu.txt wants the file
    if d:
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "parity_margins_linear24_glu.txt")   # shared with tests/test_gpu_linear24_glu.py: each keeps the other's lines
        kept = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        with open(path, "w") as fh:
            fh.write("\n".join([l for l in kept if not l.startswith(TAG)] + lines) + "\n")


# ------------------------------------------------------------------------------------------------ 4. SiLU alone
def test_silu_alone_is_inside_its_derived_bound(gpu):
    """hidden 16, in 64, 65536 tokens, fp32 out.  Gate row: weights 1 at columns 2 and 3; X[t] = (0, 0, 0, 1, 0, ..): acc_g = 1 and
    g = x_scale[t] exactly (the gate bias is 0).  u is held at exactly 1 by the up BIAS over a zero accumulator (up rows: weights 1 at
    columns 0 and 1, where X is 0) -- x_scale multiplies u's accumulator too, so a single-1 up row would make u = x_scale[t].  Then
    Y = a * 1 = a.  x_scale sweeps random mantissas in every binade of +-[2^-30, 2^7], +-0, +-88, +-89, +-104; NaN and +-inf gates
    enter through X itself (e5m2) at x_scale 1 so that u stays 1: NaN -> NaN, +inf -> +inf, -inf -> -0.  x_scale = +-inf / NaN
    make u = inf * 0 + 1 = NaN: Y is NaN.
    Bound (derived, not measured): |a - silu64(g)| <= 4 * 2^-24 |silu64(g)| + 2^-120."""
    pkg = gpu
    tokens, hidden, inf, fw, fx = 65536, 16, 64, "e4m3", "e5m2"
    assert pkg.linear24_glu_form(tokens, hidden, inf) in ("tile64", "tile128x64", "tile128")
    rng = np.random.default_rng(4)
    Wn = np.zeros((2 * hidden, inf))
    Wn[:hidden, 2:4] = 1.0
    Wn[hidden:, 0:2] = 1.0
    xb = np.zeros((tokens, inf), dtype=np.uint8)
    xb[:, 3] = encode8(np.ones(1), fx)[0]
    special = np.array([0.0, -0.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0], dtype=np.float32)
    n = tokens - len(special) - 6
    expo = rng.integers(-30, 7, size=n)            # binades [2^-30, 2^-29) .. [2^6, 2^7)
    xs = np.ldexp(rng.uniform(1.0, 2.0, n), expo).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=n)
    assert set(np.unique(expo)) == set(range(-30, 7))
    xs = np.concatenate([xs, special, np.array([np.inf, -np.inf, np.nan, 1.0, 1.0, 1.0], dtype=np.float32)])
    xb[-3, 3], xb[-2, 3], xb[-1, 3] = 0x7C, 0xFC, 0x7E          # e5m2 +inf, -inf, NaN in X
    bias = np.zeros(2 * hidden, dtype=np.float32)
    bias[hidden:] = 1.0
    blob = compress(pkg, encode8(Wn, fw), fw)
    got = glu(pkg, blob, xb, fw, fx, "f32", tokens, hidden, inf, "silu", xs=f32dev(xs), bias=f32dev(bias)).cpu().numpy()
    g = xs.astype(np.float64)[:-6]
    a, ref = got[:-6].astype(np.float64), silu64(g)[:, None]
    assert np.isfinite(a).all()
    ratio = np.abs(a - ref) / (4.0 * 2.0 ** -24 * np.abs(ref) + 2.0 ** -120)
    worst = int(np.argmax(ratio.max(axis=1)))
    what = f"silu alone: 65530 gates, worst at g = {float(g[worst])!r}"
    print(f"{what}: err / bound = {float(ratio.max()):.4f}")
    note_margin("silu alone", float(ratio.max()), what)
    assert float(ratio.max()) <= 1.0, what
    cut = g < -89.0                                # e = +inf: exactly -0
    assert cut.any() and np.array_equal(a[cut].view(np.int64), np.full(a[cut].shape, -0.0).view(np.int64))
    assert np.isnan(got[-6:-3]).all()                                             # x_scale +-inf, NaN: u = NaN
    assert (got[-3] == np.inf).all() and np.isnan(got[-1]).all()                  # g = +inf, NaN
    assert np.array_equal(got[-2].view(np.int32), np.full(hidden, -0.0, dtype=np.float32).view(np.int32))   # g = -inf: a = -0, y = -0 * 1


# ------------------------------------------------------------------------------------------------ 5. all acts against fp64
@pytest.mark.parametrize("o", OUTS)
@pytest.mark.parametrize("tokens,want", [(8, "decode"), (200, "tile64")])
def test_all_acts_against_fp64_with_bias_and_scales(gpu, tokens, want, o):
    """|y - y64| <= ROUND |y64| + L E_g |u64| + |a64| E_u + L E_g E_u + 6 * 2^-24 |a64 u64| + 2^-120 |u64| + TINY, L = 1.1 for SiLU
    (|silu'| <= 1.0999) and 1 otherwise, E = (2 in + U_OPS) 2^-24 S the accumulator bound of tests/test_gpu_linear24_fp8.py for each
    half (S = |s| sum |w x| + |bias|)."""
    pkg = gpu
    hidden, inf = 164, 256
    check_form(pkg, tokens, hidden, inf, want)
    for fw, fx in (("e4m3", "e4m3"), ("e5m2", "e4m3")):
        wb, xb = rand_bytes((tokens, hidden, inf), fw, fx, 500 + tokens)
        rng = np.random.default_rng(550 + tokens + OUTS.index(o))
        ws, xs = rng.uniform(0.5, 2.0, 2 * hidden).astype(np.float32), rng.uniform(0.5, 2.0, tokens).astype(np.float32)
        bias = rng.uniform(-2, 2, 2 * hidden).astype(np.float32)
        W64, X64 = decode8(wb, fw), decode8(xb, fx)
        s = ws.astype(np.float64)[None, :] * xs.astype(np.float64)[:, None]
        v = s * (X64 @ W64.T) + bias.astype(np.float64)[None, :]
        E = (2.0 * inf + U_OPS) * 2.0 ** -24 * (s * (np.abs(X64) @ np.abs(W64).T) + np.abs(bias.astype(np.float64))[None, :])
        g64, u64, Eg, Eu = v[:, :hidden], v[:, hidden:], E[:, :hidden], E[:, hidden:]
        blob, Xp = compress(pkg, wb, fw), padded_x(xb, fx)
        for act in ACTS:
            L = 1.1 if act == "silu" else 1.0
            a64 = act64(g64, act)
            y64 = a64 * u64
            bound = (ROUND[o] * np.abs(y64) + L * Eg * np.abs(u64) + np.abs(a64) * Eu + L * Eg * Eu + 6.0 * 2.0 ** -24 * np.abs(y64)
                     + 2.0 ** -120 * np.abs(u64) + TINY[o])
            got = glu(pkg, blob, xb, fw, fx, o, tokens, hidden, inf, act, f32dev(ws), f32dev(xs), f32dev(bias), Xp).double().cpu().numpy()
            ratio = float((np.abs(got - y64) / bound).max())
            what = f"{want} {fw} x {fx} -> {o} tokens {tokens} {act}"
            print(f"{what}: err / bound = {ratio:.4f}")
            note_margin(f"{want} {act}", ratio, what)
            assert np.isfinite(got).all() and ratio <= 1.0, what


# ------------------------------------------------------------------------------------------------ 6. special values, repeat, graph
@pytest.mark.parametrize("fw,fx", [("e5m2", "e5m2"), ("e4m3", "e4m3")])
@pytest.mark.parametrize("tokens,want", [(5, "decode"), (40, "tile64")])
def test_nan_inf_reach_exactly_the_outputs_they_feed_and_runs_repeat(gpu, tokens, want, fw, fx):
    pkg = gpu
    hidden, inf = 48, 256
    check_form(pkg, tokens, hidden, inf, want)
    wb, xb = (a.copy() for a in rand_bytes((tokens, hidden, inf), fw, fx, 600 + tokens, 0.25))
    kept = lambda row, n: int(np.flatnonzero(wb[row] & 0x7F)[n])
    wb[9, kept(9, 1)] = NAN_BYTE[fw]                       # gate row 9
    xb[0, 17] = NAN_BYTE[fx]
    if fw == "e5m2":
        wb[hidden + 7, kept(hidden + 7, 2)] = 0x7C         # +inf in up row 7
    if fx == "e5m2":
        xb[1, 33], xb[2, 70] = 0x7C, 0xFC                  # +inf, -inf
    W64, X64 = decode8(wb, fw), decode8(xb, fx)
    keptm = (wb & 0x7F) != 0                               # every kept byte is non-zero (wlo = 0.25), every dropped one zero
    with np.errstate(invalid="ignore"):
        acc = np.stack([np.where(keptm, W64 * X64[t][None, :], 0.0).sum(axis=1) for t in range(tokens)])
    feeds = (~np.isfinite(X64)).astype(np.int64) @ keptm.T.astype(np.int64) + (~np.isfinite(W64)).any(axis=1)[None, :]
    assert np.array_equal(~np.isfinite(acc), feeds > 0)
    g64, u64 = acc[:, :hidden], acc[:, hidden:]
    blob, Xp = compress(pkg, wb, fw), padded_x(xb, fx)
    got = glu(pkg, blob, xb, fw, fx, "f32", tokens, hidden, inf, "none", Xp=Xp)
    again = glu(pkg, blob, xb, fw, fx, "f32", tokens, hidden, inf, "none", Xp=Xp)
    assert torch.equal(bits(got), bits(again)), "two runs on the same inputs differ"
    # bilinear: an output is non-finite exactly when a NaN / inf reached its g or its u through a KEPT position
    fed = (feeds[:, :hidden] + feeds[:, hidden:]) > 0
    assert fed.any() and not fed.all()
    assert np.array_equal(~np.isfinite(got.cpu().numpy()), fed)
    # SiLU and ReLU: NaN stays NaN, a +inf gate gives +-inf (NaN on u = 0), a -inf gate a (signed) zero; the class of every output is fp64's
    for act in ("silu", "relu"):
        y = glu(pkg, blob, xb, fw, fx, "f32", tokens, hidden, inf, act, Xp=Xp).cpu().numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            a64 = np.where(g64 == -np.inf, -0.0, act64(g64, act)) if act == "silu" else np.where(np.isnan(g64), g64, np.maximum(g64, 0.0))
            y64 = a64 * u64
        assert np.array_equal(np.isnan(y), np.isnan(y64)), act
        assert np.array_equal(np.isinf(y), np.isinf(y64)) and np.array_equal(y[np.isinf(y64)], y64[np.isinf(y64)].astype(np.float32)), act
        if fx == "e5m2":
            neg = (g64 == -np.inf) & np.isfinite(u64)
            assert neg.any() and bool((y[neg] == 0.0).all()), act


@pytest.mark.parametrize("tokens,want", [(8, "decode"), (200, "tile64")])
def test_hipgraph_replay_gives_the_eager_bits(gpu, tokens, want):
    pkg = gpu
    hidden, inf, fw, fx, o = 256, 512, "e4m3", "e4m3", "bf16"
    check_form(pkg, tokens, hidden, inf, want)
    wb, xb = rand_bytes((tokens, hidden, inf), fw, fx, 700 + tokens)
    rng = np.random.default_rng(750 + tokens)
    blob, X = compress(pkg, wb, fw), dev8(xb, fx)
    ws, xs, bias = f32dev(rng.uniform(0.5, 2.0, 2 * hidden)), f32dev(rng.uniform(0.5, 2.0, tokens)), f32dev(rng.uniform(-1, 1, 2 * hidden))
    eager = torch.full((tokens, hidden), 9.0, dtype=ODT[o], device=DEV)
    pkg.linear24_glu_fp8(blob, X, eager, tokens, hidden, inf, w_scale=ws, x_scale=xs, bias=bias)
    torch.cuda.synchronize()
    Y = torch.full((tokens, hidden), 5.0, dtype=ODT[o], device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):      # one stream, one kernel node: no parallel branches
        pkg.linear24_glu_fp8(blob, X, Y, tokens, hidden, inf, w_scale=ws, x_scale=xs, bias=bias)
    Y.fill_(5.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(Y), bits(eager))
