"""sm_linear24_glu_{f16,bf16} on the device: Y[tokens][hidden] = act(g) * u with g, u the two halves of a fused gate/up 2:4 weight,
token-major in and out, one launch.  The reference is this file's own numpy fp64 on the 16-bit operands.

1. each half alone (the other held at exactly 1) equals the matching columns of sm_linear24_* on the same blob bit for bit: the row
   map, the clamps and both accumulators of every tile instantiation and of the decode form;
3. integer operands: the fp64 product rounded once to the output type, bit for bit, every form and type;
5. every activation against fp64 with a bias, decode and a tile form per type;
6. NaN / inf reach exactly the outputs they feed; two runs and a hipGraph replay give the same bits;
7. spmma_plan_t::linear_glu through the C++ headers (examples/bin/linear24_glu).
(2. and 4. -- fp32 out, SiLU alone -- need an fp32 output: tests/test_gpu_linear24_glu_fp8.py.)
Every call runs on X with ldx > in and NaN in the padding and behind the last token, and on Y with ldy > hidden whose slack columns
and tail row are guarded by a sentinel.  Every test named for a form asks linear24_glu_form -- at the 256 compute units the 16-bit
layer asks it with -- which form its shape runs."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
from linear24_testlib import CUS, DEV, DT, INT_SHAPES, SENTINEL, SHAPES, SID, TYPES, act64, f32dev, mask24, todev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}
ACTS = ["none", "relu", "silu"]
U_OPS = 1      # fp32 operations between an accumulator and the gate: the bias add (s = 1)


def bits(t):
    return t.contiguous().view(torch.int16)


def compress(pkg, W):
    rows, inf = W.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 2, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24(W.contiguous(), rows, inf, inf, 1, rows * inf, blob)
    return blob


def check_form(pkg, tokens, hidden, inf, want):
    assert pkg.linear24_glu_form(tokens, hidden, inf, cus=CUS) == want
    assert pkg.linear24_fp8_form(tokens, 2 * hidden, inf, cus=CUS) == want      # the plain rule on 2 * hidden rows: the same blob, the same form


def padded_x(X):
    """[tokens + 1][in + 16] with NaN in the padding and in the row behind the last token"""
    tokens, inf = X.shape
    Xp = torch.full((tokens + 1, inf + 16), float("nan"), dtype=X.dtype, device=DEV)
    Xp[:tokens, :inf] = X
    return Xp, inf + 16


def glu(pkg, blob, Xp, tokens, hidden, inf, act, bias=None):
    """The gated call on padded X and a sentinel-guarded Y; returns Y[:tokens, :hidden] (a copy)."""
    X, ldx = Xp
    ldy = hidden + 12
    Y = torch.full((tokens + 1, ldy), SENTINEL, dtype=X.dtype, device=DEV)
    pkg.linear24_glu(blob, X, Y, tokens, hidden, inf, act=act, bias=bias, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    assert bool((Y[:tokens, hidden:] == SENTINEL).all()) and bool((Y[tokens] == SENTINEL).all()), "slack columns or the tail row of Y were written"
    return Y[:tokens, :hidden].contiguous()


def plain(pkg, blob, Xp, tokens, hidden, inf):
    """sm_linear24_* on the same blob: [tokens][2 hidden]"""
    X, ldx = Xp
    Y = torch.full((tokens, 2 * hidden), SENTINEL, dtype=X.dtype, device=DEV)
    pkg.linear24(blob, X, Y, tokens, 2 * hidden, inf, ldx=ldx)
    torch.cuda.synchronize()
    return Y


@functools.lru_cache(maxsize=None)
def rand_operands(shape, seed, wlo=0.0):
    """W[2 hidden][in] 2:4 with the kept values in U(-2, 2) (wlo = 0.25: |w| >= 0.25, no kept value is zero), X in U(-2, 2): fp64"""
    tokens, hidden, inf = shape
    rng = np.random.default_rng(seed)
    w = rng.uniform(wlo, 2.0, (2 * hidden, inf)) * rng.choice(np.array([-1.0, 1.0]), size=(2 * hidden, inf))
    return np.where(mask24(rng, 2 * hidden, inf), w, 0.0), rng.uniform(-2, 2, (tokens, inf))


# ------------------------------------------------------------------------------------------------ 1. each half against the plain layer
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
@pytest.mark.parametrize("ty", TYPES)
def test_each_half_equals_the_plain_layer_bit_for_bit(gpu, ty, shape):
    """Up rows = a single 1 at column 0 and X[:, 0] = 1 make u exactly 1: with act NONE Y is g, which must be columns 0 .. hidden-1 of
    sm_linear24_* on the same blob; mirrored with the gate rows held at 1, Y is u = columns hidden .. 2 hidden - 1."""
    pkg = gpu
    tokens, hidden, inf, want = shape
    check_form(pkg, tokens, hidden, inf, want)
    Wn, Xn = rand_operands(shape[:3], 100 + SHAPES.index(shape))
    Xn = Xn.copy()
    Xn[:, 0] = 1.0
    Xp = padded_x(todev(Xn, ty))
    for half, cols in ((1, slice(0, hidden)), (0, slice(hidden, 2 * hidden))):    # the half held at 1, the columns Y must equal
        Wh = Wn.copy()
        Wh[half * hidden:(half + 1) * hidden] = 0.0
        Wh[half * hidden:(half + 1) * hidden, 0] = 1.0
        blob = compress(pkg, todev(Wh, ty))
        got = glu(pkg, blob, Xp, tokens, hidden, inf, "none")
        ref = plain(pkg, blob, Xp, tokens, hidden, inf)
        assert bool((ref[:, half * hidden:(half + 1) * hidden] == 1.0).all())
        bad = torch.nonzero(bits(got) != bits(ref[:, cols]))
        assert bad.numel() == 0, f"{'gate' if half else 'up'} half: first mismatch at (token, feature) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


# ------------------------------------------------------------------------------------------------ 3. integer-exact
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_operands_give_the_fp64_product_rounded_once(gpu, shape, ty):
    """W in {-1, 0, 1} (two kept of four), X integers in [-3, 3], in = 64: |g|, |u| <= 32 * 3 = 96, so g, u and g * u <= 9216 are exact
    in fp32 and finite in fp16; Y is the fp64 product rounded ONCE to the output type (integers that large are exact in neither
    16-bit type: the rounding is part of the comparison)."""
    pkg = gpu
    tokens, hidden, want = shape
    inf = 64
    check_form(pkg, tokens, hidden, inf, want)
    rng = np.random.default_rng(300 + 10 * INT_SHAPES.index(shape) + TYPES.index(ty))
    Wn = np.where(mask24(rng, 2 * hidden, inf), rng.choice(np.array([-1.0, 1.0]), size=(2 * hidden, inf)), 0.0)
    Xn = rng.integers(-3, 4, size=(tokens, inf)).astype(np.float64)
    acc = Xn @ Wn.T
    g, u = acc[:, :hidden], acc[:, hidden:]
    assert np.abs(acc).max() <= 96
    blob, Xp = compress(pkg, todev(Wn, ty)), padded_x(todev(Xn, ty))
    for act in ("none", "relu"):
        ref = torch.from_numpy((g if act == "none" else np.maximum(g, 0.0)) * u).to(DT[ty])     # integers: fp64 -> fp32 is exact, one rounding follows
        got = glu(pkg, blob, Xp, tokens, hidden, inf, act).cpu()
        bad = torch.nonzero(bits(got) != bits(ref))
        assert bad.numel() == 0, f"{act} -> {ty}: first mismatch at {bad[0].tolist()}: got {float(got[tuple(bad[0])])}, want {float(ref[tuple(bad[0])])}"


# ------------------------------------------------------------------------------------------------ margins
MARGINS = {}
TAG = "[16-bit]"


def note_margin(key, ratio, what):
    if key not in MARGINS or ratio > MARGINS[key][0]:
        MARGINS[key] = (ratio, what)


@pytest.fixture(scope="module", autouse=True)
def _margin_report():
    yield
    if not MARGINS:
        return
    lines = [f"{TAG}{key:14s} {r:.4f}  {what}" for key, (r, what) in sorted(MARGINS.items())]
    print("\n".join(["sm_linear24_glu_{f16,bf16}: worst err / bound"] + lines))
    d = os.environ.get("SM_PARITY_MARGINS_DIR")   # where a run that refreshes profiles/parity_margins_linear24_glu.txt wants the file
    if d:
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "parity_margins_linear24_glu.txt")   # shared with tests/test_gpu_linear24_glu_fp8.py: each keeps the other's lines
        kept = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        with open(path, "w") as fh:
            fh.write("\n".join([l for l in kept if not l.startswith(TAG)] + lines) + "\n")


# ------------------------------------------------------------------------------------------------ 5. all acts against fp64
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("tokens,want", [(8, "decode"), (200, "tile64")])
def test_all_acts_against_fp64_with_bias(gpu, tokens, want, ty):
    """|y - y64| <= ROUND |y64| + L E_g |u64| + |a64| E_u + L E_g E_u + 6 * 2^-24 |a64 u64| + 2^-120 |u64| + TINY, L = 1.1 for SiLU
    (|silu'| <= 1.0999) and 1 otherwise, E = (2 in + U_OPS) 2^-24 S the accumulator bound of tests/test_gpu_linear24.py for each half
    (S = sum |w x| + |bias|; U_OPS = 1, the bias add)."""
    pkg = gpu
    hidden, inf = 164, 256
    check_form(pkg, tokens, hidden, inf, want)
    Wn, Xn = rand_operands((tokens, hidden, inf), 500 + tokens)
    W, X = todev(Wn, ty), todev(Xn, ty)
    W64, X64 = W.double().cpu().numpy(), X.double().cpu().numpy()
    rng = np.random.default_rng(550 + tokens + TYPES.index(ty))
    bias = rng.uniform(-2, 2, 2 * hidden).astype(np.float32)
    v = X64 @ W64.T + bias.astype(np.float64)[None, :]
    E = (2.0 * inf + U_OPS) * 2.0 ** -24 * (np.abs(X64) @ np.abs(W64).T + np.abs(bias.astype(np.float64))[None, :])
    g64, u64, Eg, Eu = v[:, :hidden], v[:, hidden:], E[:, :hidden], E[:, hidden:]
    blob, Xp = compress(pkg, W), padded_x(X)
    for act in ACTS:
        L = 1.1 if act == "silu" else 1.0
        a64 = act64(g64, act)
        y64 = a64 * u64
        bound = (ROUND[ty] * np.abs(y64) + L * Eg * np.abs(u64) + np.abs(a64) * Eu + L * Eg * Eu + 6.0 * 2.0 ** -24 * np.abs(y64)
                 + 2.0 ** -120 * np.abs(u64) + TINY[ty])
        got = glu(pkg, blob, Xp, tokens, hidden, inf, act, f32dev(bias)).double().cpu().numpy()
        ratio = float((np.abs(got - y64) / bound).max())
        what = f"{want} {ty} tokens {tokens} {act}"
        print(f"{what}: err / bound = {ratio:.4f}")
        note_margin(f"{want} {act}", ratio, what)
        assert np.isfinite(got).all() and ratio <= 1.0, what


# ------------------------------------------------------------------------------------------------ 6. special values, repeat, graph
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("tokens,want", [(5, "decode"), (40, "tile64")])
def test_nan_inf_reach_exactly_the_outputs_they_feed_and_runs_repeat(gpu, tokens, want, ty):
    pkg = gpu
    hidden, inf = 48, 256
    check_form(pkg, tokens, hidden, inf, want)
    Wn, Xn = (a.copy() for a in rand_operands((tokens, hidden, inf), 600 + tokens, 0.25))
    keptm = Wn != 0.0                                      # every kept value is non-zero (wlo = 0.25, far above either type's underflow)
    kept = lambda row, n: int(np.flatnonzero(keptm[row])[n])
    Wn[9, kept(9, 1)] = np.nan                             # gate row 9
    Wn[hidden + 7, kept(hidden + 7, 2)] = np.inf           # up row 7
    Xn[0, 17], Xn[1, 33], Xn[2, 70] = np.nan, np.inf, -np.inf
    W, X = todev(Wn, ty), todev(Xn, ty)
    W64, X64 = W.double().cpu().numpy(), X.double().cpu().numpy()
    with np.errstate(invalid="ignore"):
        acc = np.stack([np.where(keptm, W64 * X64[t][None, :], 0.0).sum(axis=1) for t in range(tokens)])
    feeds = (~np.isfinite(X64)).astype(np.int64) @ keptm.T.astype(np.int64) + (~np.isfinite(W64)).any(axis=1)[None, :]
    assert np.array_equal(~np.isfinite(acc), feeds > 0)
    g64, u64 = acc[:, :hidden], acc[:, hidden:]
    blob, Xp = compress(pkg, W), padded_x(X)
    got = glu(pkg, blob, Xp, tokens, hidden, inf, "none")
    again = glu(pkg, blob, Xp, tokens, hidden, inf, "none")
    assert torch.equal(bits(got), bits(again)), "two runs on the same inputs differ"
    # bilinear: an output is non-finite exactly when a NaN / inf reached its g or its u through a KEPT position
    fed = (feeds[:, :hidden] + feeds[:, hidden:]) > 0
    assert fed.any() and not fed.all()
    assert np.array_equal(~np.isfinite(got.float().cpu().numpy()), fed)
    # SiLU and ReLU: NaN stays NaN, a +inf gate gives +-inf (NaN on u = 0), a -inf gate a (signed) zero; the class of every output is fp64's
    for act in ("silu", "relu"):
        y = glu(pkg, blob, Xp, tokens, hidden, inf, act).float().cpu().numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            a64 = np.where(g64 == -np.inf, -0.0, act64(g64, act)) if act == "silu" else np.where(np.isnan(g64), g64, np.maximum(g64, 0.0))
            y64 = a64 * u64
        assert np.array_equal(np.isnan(y), np.isnan(y64)), act
        assert np.array_equal(np.isinf(y), np.isinf(y64)) and np.array_equal(y[np.isinf(y64)], y64[np.isinf(y64)].astype(np.float32)), act
        neg = (g64 == -np.inf) & np.isfinite(u64)
        assert neg.any() and bool((y[neg] == 0.0).all()), act


@pytest.mark.parametrize("tokens,want", [(8, "decode"), (200, "tile64")])
def test_hipgraph_replay_gives_the_eager_bits(gpu, tokens, want):
    pkg = gpu
    hidden, inf, ty = 256, 512, "bf16"
    check_form(pkg, tokens, hidden, inf, want)
    Wn, Xn = rand_operands((tokens, hidden, inf), 700 + tokens)
    blob, X = compress(pkg, todev(Wn, ty)), todev(Xn, ty)
    bias = f32dev(np.random.default_rng(750 + tokens).uniform(-1, 1, 2 * hidden))
    eager = torch.full((tokens, hidden), 9.0, dtype=DT[ty], device=DEV)
    pkg.linear24_glu(blob, X, eager, tokens, hidden, inf, bias=bias)
    torch.cuda.synchronize()
    Y = torch.full((tokens, hidden), 5.0, dtype=DT[ty], device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):      # one stream, one kernel node: no parallel branches
        pkg.linear24_glu(blob, X, Y, tokens, hidden, inf, bias=bias)
    Y.fill_(5.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(Y), bits(eager))


# ------------------------------------------------------------------------------------------------ 7. the C++ header mirror
@pytest.mark.parametrize("hidden,inf,tokens", [(328, 320, 200), (4096, 4096, 8)])
def test_cpp_header_mirror(gpu, hidden, inf, tokens):
    """spmma_plan_t::linear_glu (include/sparsify.me/spmma.hxx) against spmma_plan_t::linear on the same blob + a host SwiGLU: the
    example checks itself and exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "linear24_glu")
    assert os.path.exists(exe), "examples/bin/linear24_glu is missing: build() makes it"
    res = subprocess.run([exe, str(hidden), str(inf), str(tokens)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "within the rounding bound" in res.stdout and "yes" in res.stdout
