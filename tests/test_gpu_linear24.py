"""sm_linear24_{f16,bf16} on the device: Y[tokens][out] = act(alpha * X . W_2:4^T + beta * R + bias), token-major in and out.

* exact integer products pin the K-contiguous X fragment and the untransposed store of both forms;
* the tile form (tokens > 16, or out > 16384) equals sm_transpose(X) + sm_spmma[_ex] + sm_transpose(C) bit for bit;
* the decode form (tokens <= 16 and out <= 16384) is held to the bound of DESIGN.md section 2 against the fp64 product on the kept positions:
  |got - ref| <= ROUND * |ref| + 2k * 2^-24 * sum|w * x|, ROUND = 2^-11 (fp16) / 2^-8 (bf16);
* NaN / inf, hipGraph replay, and the C++ header path."""
import csv
import os
import subprocess

import numpy as np
import pytest
import torch
from linear24_testlib import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {False: torch.float16, True: torch.bfloat16}
ROUND = {False: 2.0 ** -11, True: 2.0 ** -8}


def table():
    lines = open(os.path.join(ROOT, "datasets", "linear_shapes.csv")).read().splitlines()
    return [(int(r["out"]), int(r["in"])) for r in csv.DictReader(l for l in lines if not l.startswith("#"))]


TABLE = table()


def bits(t):
    return t.view(torch.int16)


def compress(pkg, W, out, inf):
    """blob of the (already 2:4) weight W[out][in]"""
    blob = torch.empty(pkg.compress24_size(out, inf, 2, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24(W, out, inf, inf, 1, out * inf, blob)
    return blob


def pruned_weight(pkg, out, inf, bf, seed, lo=-2.0, hi=2.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = (torch.rand(out, inf, generator=g, device=DEV) * (hi - lo) + lo).to(DT[bf])
    pkg.prune24(W, W, out, inf, inf, pkg.PRUNE_STRIP)
    return W


def rand(shape, bf, seed, lo=-2.0, hi=2.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(*shape, generator=g, device=DEV) * (hi - lo) + lo).to(DT[bf])


def route(pkg, blob, X, tokens, out, inf, ldx=None, alpha=1.0, beta=0.0, R=None, epilogue=None):
    """What a caller ran before: transpose X, the 2:4 matmul with W as A, transpose the result.  R: [tokens][out] contiguous, or None.
    `epilogue` is given in the ROUTE's coordinates (C[out][tokens])."""
    ldx = inf if ldx is None else ldx
    Xt = torch.empty(inf, tokens, dtype=X.dtype, device=DEV)
    pkg.transpose(X, Xt, tokens, inf, ld_in=ldx, ld_out=tokens)
    C = torch.full((out, tokens), 3.0, dtype=X.dtype, device=DEV)
    if R is not None:
        pkg.transpose(R, C, tokens, out, ld_in=out, ld_out=tokens)  # in place in the route: C holds R^T
    pkg.spmma(blob, Xt, C, out, tokens, inf, alpha=alpha, beta=beta, epilogue=epilogue)
    Y = torch.empty(tokens, out, dtype=X.dtype, device=DEV)
    pkg.transpose(C, Y, out, tokens, ld_in=tokens, ld_out=out)
    torch.cuda.synchronize()
    return Y


# ------------------------------------------------------------------------------------------------ lane maps, exact
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("out", [16, 100, 130, 4096])
@pytest.mark.parametrize("tokens", [1, 3, 16, 17, 64, 200])
def test_integer_products_are_exact(gpu, bf, out, tokens):
    """W: two of every four kept, values in {-2, -1, 1, 2}; X in {-1, 0, 1}; in = 128: |y| <= 64 * 2 = 2^7, every partial sum an exact
    fp32 integer in any order, every output exact in fp16 and in bf16."""
    pkg, inf = gpu, 128
    rng = np.random.default_rng(1000 * out + tokens + (7 if bf else 0))
    Wn = np.zeros((out, inf // 4, 4), dtype=np.int64)
    keep = np.argsort(rng.random((out, inf // 4, 4)), axis=2)[:, :, :2]
    vals = rng.choice(np.array([-2, -1, 1, 2]), size=(out, inf // 4, 2))
    np.put_along_axis(Wn, keep, vals, axis=2)
    Wn = Wn.reshape(out, inf)
    Xn = rng.integers(-1, 2, size=(tokens, inf))
    ref = Xn @ Wn.T
    assert np.abs(ref).max() <= 2 ** 7
    W = torch.from_numpy(Wn).to(DT[bf]).to(DEV)
    X = torch.from_numpy(Xn).to(DT[bf]).to(DEV)
    blob = compress(pkg, W, out, inf)
    Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, X, Y, tokens, out, inf)
    torch.cuda.synchronize()
    got = Y.double().cpu().numpy()
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"first mismatch at (token, out) {bad[0]}: got {got[tuple(bad[0])]}, want {ref[tuple(bad[0])]}; {len(bad)} of {ref.size}"


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("out", [16, 100])
@pytest.mark.parametrize("tokens", [3, 16])
def test_decode_k_split_is_exact_on_integers(gpu, bf, out, tokens):
    """in = 64 * (16 * 4 + 1): every one of the decode form's 16 waves multiplies, with a full look-ahead batch of four stages and a
    ragged fifth trip.  X has exactly one +-1 per 64-k stage (65 per row), W as above: |y| <= 130 < 2^8, exact in any order."""
    pkg, inf = gpu, 64 * 65
    rng = np.random.default_rng(77 * out + tokens + (5 if bf else 0))
    Wn = np.zeros((out, inf // 4, 4), dtype=np.int64)
    keep = np.argsort(rng.random((out, inf // 4, 4)), axis=2)[:, :, :2]
    np.put_along_axis(Wn, keep, rng.choice(np.array([-2, -1, 1, 2]), size=(out, inf // 4, 2)), axis=2)
    Wn = Wn.reshape(out, inf)
    Xn = np.zeros((tokens, 65, 64), dtype=np.int64)
    pos = rng.integers(0, 64, size=(tokens, 65, 1))
    np.put_along_axis(Xn, pos, rng.choice(np.array([-1, 1]), size=(tokens, 65, 1)), axis=2)
    Xn = Xn.reshape(tokens, inf)
    ref = Xn @ Wn.T
    assert np.abs(ref).max() <= 2 ** 8
    W = torch.from_numpy(Wn).to(DT[bf]).to(DEV)
    X = torch.from_numpy(Xn).to(DT[bf]).to(DEV)
    blob = compress(pkg, W, out, inf)
    Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, X, Y, tokens, out, inf)
    torch.cuda.synchronize()
    assert np.array_equal(Y.double().cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ tile form == the three-call route
TILE_SHAPES = [  # tokens, out, in
    (128, 128, 128),      # one tile
    (17, 64, 64),         # the smallest tile-form call
    (200, 328, 192),      # ragged in both dimensions
    (77, 130, 256),       # out % 4 != 0: the per-element store
    (333, 516, 320),
]


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_tile_form_equals_the_route(gpu, shape, bf):
    pkg = gpu
    tokens, out, inf = shape
    W = pruned_weight(pkg, out, inf, bf, 11)
    blob = compress(pkg, W, out, inf)
    X = rand((tokens, inf), bf, 12)
    Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, X, Y, tokens, out, inf)
    ref = route(pkg, blob, X, tokens, out, inf)
    assert torch.equal(bits(Y), bits(ref))
    # alpha, beta (NULL epilogue: beta reads Y)
    R = rand((tokens, out), bf, 13)
    Y2 = R.clone()
    pkg.linear24(blob, X, Y2, tokens, out, inf, alpha=0.75, beta=-1.25)
    ref2 = route(pkg, blob, X, tokens, out, inf, alpha=0.75, beta=-1.25, R=R)
    assert torch.equal(bits(Y2), bits(ref2))


@pytest.mark.parametrize("bf", [False, True])
def test_leading_dimensions_and_slack_columns(gpu, bf):
    pkg = gpu
    tokens, out, inf, ldx, ldy = 150, 256, 192, 200, 300
    W = pruned_weight(pkg, out, inf, bf, 21)
    blob = compress(pkg, W, out, inf)
    Xp = rand((tokens, ldx), bf, 22)
    Yp = torch.full((tokens, ldy), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, Xp, Yp, tokens, out, inf, ldx=ldx, ldy=ldy)
    ref = route(pkg, blob, Xp, tokens, out, inf, ldx=ldx)
    assert torch.equal(bits(Yp[:, :out].contiguous()), bits(ref))
    assert bool((Yp[:, out:] == 9.0).all()), "the slack columns of Y were written"
    # a column slice of a wider buffer whose start is only 2-byte aligned: the per-element store
    Yq = torch.full((tokens, ldy), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, Xp, Yq.view(-1)[3:], tokens, out, inf, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    assert torch.equal(bits(Yq[:, 3:3 + out].contiguous()), bits(ref))
    assert bool((Yq[:, :3] == 9.0).all()) and bool((Yq[:, 3 + out:] == 9.0).all())


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", TABLE)
def test_table_shapes_at_512_tokens_equal_the_route(gpu, shape, bf):
    pkg = gpu
    out, inf = shape
    tokens = 512
    W = pruned_weight(pkg, out, inf, bf, 31)
    blob = compress(pkg, W, out, inf)
    del W
    X = rand((tokens, inf), bf, 32)
    Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, X, Y, tokens, out, inf)
    ref = route(pkg, blob, X, tokens, out, inf)
    assert torch.equal(bits(Y), bits(ref))


# the shapes that reach the two larger tiles (the rule: 128 x 128 when it gives >= 256 workgroups and tokens > 64, else 128 x 64 when
# that gives >= 256): ragged in both dimensions, out % 4 != 0 (per-element store), ldy > out
LARGE_TILE_SHAPES = [(300, 16390, 128), (260, 8198, 128), (300, 16392, 192), (260, 8200, 192)]


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", LARGE_TILE_SHAPES)
def test_large_tiles_ragged_with_epilogues_equal_the_route(gpu, shape, bf):
    """128 x 128 (first and third shape) and 128 x 64 tiles: edge clamps of the three DMA streams, the store guards, the per-element
    (out % 4 != 0) and the packed (out % 4 == 0) store with ldy > out, alpha / beta, residual R != Y, both bias maps with an activation."""
    pkg = gpu
    tokens, out, inf = shape
    assert -(-out // 128) * -(-tokens // (128 if tokens > 260 else 64)) >= 256
    ldy = out + 12
    W = pruned_weight(pkg, out, inf, bf, 91)
    blob = compress(pkg, W, out, inf)
    X = rand((tokens, inf), bf, 92, -1.0, 1.0)
    R = rand((tokens, out), bf, 93, -8.0, 8.0)
    Rp = torch.full((tokens, ldy), 7.0, dtype=DT[bf], device=DEV)      # R with Y's leading dimension
    Rp[:, :out] = R
    Rt = torch.empty(out, tokens, dtype=DT[bf], device=DEV)
    pkg.transpose(R, Rt, tokens, out, ld_in=out, ld_out=tokens)
    b_out = (torch.rand(out, device=DEV) * 4 - 2).float()
    b_tok = (torch.rand(tokens, device=DEV) * 4 - 2).float()

    def check(ref, what, **kw):
        Yp = torch.full((tokens, ldy), 9.0, dtype=DT[bf], device=DEV)
        pkg.linear24(blob, X, Yp, tokens, out, inf, ldy=ldy, **kw)
        torch.cuda.synchronize()
        assert torch.equal(bits(Yp[:, :out].contiguous()), bits(ref)), what
        assert bool((Yp[:, out:] == 9.0).all()), what + ": slack columns written"

    check(route(pkg, blob, X, tokens, out, inf), "plain")
    # NULL epilogue, beta reads Y: covered through R == Y below; here alpha / beta with R != Y
    check(route(pkg, blob, X, tokens, out, inf, alpha=0.75, beta=-1.25, R=R), "alpha beta residual",
          alpha=0.75, beta=-1.25, epilogue=pkg.Epilogue(residual=Rp))
    for act, arg in (("relu", 0.0), ("hardswish", 0.0), ("leaky_relu", 0.1)):
        for mine_dim, bias, route_dim in (("col", b_out, "row"), ("row", b_tok, "col")):
            ref = route(pkg, blob, X, tokens, out, inf, alpha=1.5, beta=0.5,
                        epilogue=pkg.Epilogue(bias=bias, bias_dim=route_dim, act=act, act_arg=arg, residual=Rt))
            check(ref, f"{act} bias {mine_dim}", alpha=1.5, beta=0.5,
                  epilogue=pkg.Epilogue(bias=bias, bias_dim=mine_dim, act=act, act_arg=arg, residual=Rp))
    # in place, R == Y with ldy
    Yp = Rp.clone()
    pkg.linear24(blob, X, Yp, tokens, out, inf, ldy=ldy, beta=1.0, epilogue=pkg.Epilogue(bias=b_out, act="relu", residual=Yp))
    ref = route(pkg, blob, X, tokens, out, inf, beta=1.0, epilogue=pkg.Epilogue(bias=b_out, bias_dim="row", act="relu", residual=Rt))
    assert torch.equal(bits(Yp[:, :out].contiguous()), bits(ref)) and bool((Yp[:, out:] == 7.0).all())


ACTS = [("none", 0.0), ("relu", 0.0), ("relu6", 6.0), ("leaky_relu", 0.1), ("hardswish", 0.0)]


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", [(200, 328, 192), (77, 130, 256)])
def test_epilogues_equal_the_route_ex(gpu, shape, bf):
    """bias per out feature <-> SM_BIAS_ROW of the route, bias per token <-> SM_BIAS_COL, each activation, residual R != Y."""
    pkg = gpu
    tokens, out, inf = shape
    W = pruned_weight(pkg, out, inf, bf, 41)
    blob = compress(pkg, W, out, inf)
    X = rand((tokens, inf), bf, 42, -1.0, 1.0)
    R = rand((tokens, out), bf, 43, -8.0, 8.0)
    Rt = torch.empty(out, tokens, dtype=DT[bf], device=DEV)
    pkg.transpose(R, Rt, tokens, out, ld_in=out, ld_out=tokens)
    b_out = (torch.rand(out, device=DEV) * 4 - 2).float()
    b_tok = (torch.rand(tokens, device=DEV) * 4 - 2).float()
    for act, arg in ACTS:
        for mine_dim, bias, route_dim in (("col", b_out, "row"), ("row", b_tok, "col")):
            for beta in (0.0, 0.5):
                Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
                pkg.linear24(blob, X, Y, tokens, out, inf, alpha=1.5, beta=beta,
                             epilogue=pkg.Epilogue(bias=bias, bias_dim=mine_dim, act=act, act_arg=arg, residual=R if beta else None))
                ref = route(pkg, blob, X, tokens, out, inf, alpha=1.5, beta=beta,
                            epilogue=pkg.Epilogue(bias=bias, bias_dim=route_dim, act=act, act_arg=arg, residual=Rt if beta else None))
                assert torch.equal(bits(Y), bits(ref)), (act, mine_dim, beta)
    # in place: R == Y
    Y = R.clone()
    pkg.linear24(blob, X, Y, tokens, out, inf, beta=1.0, epilogue=pkg.Epilogue(bias=b_out, act="relu", residual=Y))
    ref = route(pkg, blob, X, tokens, out, inf, beta=1.0, epilogue=pkg.Epilogue(bias=b_out, bias_dim="row", act="relu", residual=Rt))
    assert torch.equal(bits(Y), bits(ref))


# ------------------------------------------------------------------------------------------------ decode form within the bound
def fp64_product(W, X):
    """X . W^T and sum |x| |w| in fp64 on the device (the dropped positions of W are zeros: they contribute nothing)."""
    Wd, Xd = W.double(), X.double()
    return Xd @ Wd.T, Xd.abs() @ Wd.abs().T


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", TABLE)
def test_decode_form_within_the_bound(gpu, shape, bf):
    pkg = gpu
    out, inf = shape
    W = pruned_weight(pkg, out, inf, bf, 51)
    blob = compress(pkg, W, out, inf)
    for tokens in (1, 8, 16):
        X = rand((tokens, inf), bf, 52 + tokens)
        Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
        pkg.linear24(blob, X, Y, tokens, out, inf)
        Y2 = torch.full((tokens, out), 5.0, dtype=DT[bf], device=DEV)
        pkg.linear24(blob, X, Y2, tokens, out, inf)
        torch.cuda.synchronize()
        assert torch.equal(bits(Y), bits(Y2)), "two calls on the same inputs differ"
        ref, mag = fp64_product(W, X)
        err = (Y.double() - ref).abs()
        tol = ROUND[bf] * ref.abs() + 2 * inf * 2.0 ** -24 * mag
        worst = float((err / tol.clamp_min(1e-300)).max())
        print(f"decode {out}x{inf} tokens {tokens} {'bf16' if bf else 'f16'}: worst err / bound = {worst:.3f}")
        assert bool((err <= tol).all()), f"tokens {tokens}: worst err / bound = {worst}"


def act_fp64(x, act, arg):
    if act == "relu":
        return x.clamp_min(0)
    if act == "relu6":
        return x.clamp(0, arg)
    if act == "leaky_relu":
        return torch.where(x >= 0, x, arg * x)
    if act == "hardswish":
        return x * (x + 3).clamp(0, 6) / 6
    return x


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", [(8, 328, 192), (13, 130, 256), (16, 4096, 1024)])
def test_decode_form_epilogues(gpu, shape, bf):
    """Against the formula restated on the fp64 product (a stricter reference than an fp32 restatement).  Bound = the decode bound on
    the accumulator carried through the formula, plus one output rounding more:
        ROUND |ref| + [ |alpha| 2k 2^-24 sum|w x| + 4 * 2^-24 (|alpha| sum|w x| + |beta R| + |bias|) ] + ROUND |ref|
    -- the 2k term on the accumulation only; the multiply by alpha, the fused multiply-add of beta R and the bias addition are three
    fp32 operations, and a fourth step is allowed for the activation's own arithmetic.  ReLU, clipped and leaky ReLU have slope <= 1;
    hardswish's slope is at most 1.5, so its input error is carried with that factor, and for it alone."""
    pkg = gpu
    tokens, out, inf = shape
    W = pruned_weight(pkg, out, inf, bf, 61)
    blob = compress(pkg, W, out, inf)
    X = rand((tokens, inf), bf, 62, -1.0, 1.0)
    R = rand((tokens, out), bf, 63, -8.0, 8.0)
    b_out = (torch.rand(out, device=DEV) * 4 - 2).float()
    b_tok = (torch.rand(tokens, device=DEV) * 4 - 2).float()
    acc, mag = fp64_product(W, X)
    alpha = 1.5
    for act, arg in ACTS:
        for dim, bias in (("col", b_out), ("row", b_tok)):
            for beta in (0.0, 0.5):
                Y = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
                pkg.linear24(blob, X, Y, tokens, out, inf, alpha=alpha, beta=beta,
                             epilogue=pkg.Epilogue(bias=bias, bias_dim=dim, act=act, act_arg=arg, residual=R if beta else None))
                torch.cuda.synchronize()
                bterm = bias.double()[None, :] if dim == "col" else bias.double()[:, None]
                pre = alpha * acc + beta * R.double() + bterm
                ref = act_fp64(pre, act, arg)
                premag = alpha * mag + abs(beta) * R.double().abs() + bterm.abs()
                slope = 1.5 if act == "hardswish" else 1.0
                tol = 2 * ROUND[bf] * ref.abs() + slope * (2 * inf * 2.0 ** -24 * alpha * mag + 4 * 2.0 ** -24 * premag)
                err = (Y.double() - ref).abs()
                assert bool((err <= tol).all()), (act, dim, beta, float((err / tol.clamp_min(1e-300)).max()))
    # in place
    Y = R.clone()
    pkg.linear24(blob, X, Y, tokens, out, inf, beta=1.0, epilogue=pkg.Epilogue(residual=Y))
    torch.cuda.synchronize()
    ref = acc + R.double()
    assert bool(((Y.double() - ref).abs() <= 2 * ROUND[bf] * ref.abs() + 2 * inf * 2.0 ** -24 * mag + 4 * 2.0 ** -24 * (mag + R.double().abs())).all())


# ------------------------------------------------------------------------------------------------ NaN / inf
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("tokens", [5, 40])
def test_nan_inf_propagate_as_in_the_route(gpu, bf, tokens):
    pkg = gpu
    out, inf = 96, 256
    W = pruned_weight(pkg, out, inf, bf, 71)
    # row 3 drops position 0 .. 3's zeros: find a dropped position of row 3 and a kept one of row 5
    dropped = int((W[3] == 0).nonzero()[0])
    kept = int((W[5] != 0).nonzero()[0])
    W[7, int((W[7] != 0).nonzero()[2])] = float("inf")     # an inf weight at a kept position
    W[9, int((W[9] != 0).nonzero()[1])] = float("nan")
    blob = compress(pkg, W, out, inf)
    rows = tokens + 24
    Xall = rand((rows, inf), bf, 72)
    Xall[tokens:] = float("nan")                             # token rows beyond `tokens`: never read into a stored output
    Xall[1, dropped] = float("inf")                          # meets a dropped position of out feature 3 (and kept ones elsewhere)
    Xall[2, kept] = float("-inf")
    Xall[0, 17] = float("nan")
    Y = torch.full((rows, out), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, Xall, Y, tokens, out, inf)
    ref = route(pkg, blob, Xall[:tokens].contiguous(), tokens, out, inf)
    got = Y[:tokens]
    assert bool((Y[tokens:] == 9.0).all())
    assert torch.equal(got.isnan(), ref.isnan())
    fin = ~ref.isnan()
    if tokens > 16:   # tile form: the route's bits
        assert torch.equal(bits(got)[fin], bits(ref)[fin])
    else:
        assert torch.equal(got.isinf(), ref.isinf()) and torch.equal(got[ref.isinf()], ref[ref.isinf()])
        ok = fin & ~ref.isinf()
        _, mag = fp64_product(torch.nan_to_num(W, nan=0.0, posinf=0.0, neginf=0.0), torch.nan_to_num(Xall[:tokens], nan=0.0, posinf=0.0, neginf=0.0))
        assert bool(((got.double() - ref.double()).abs()[ok] <= (2 * ROUND[bf] * ref.double().abs() + 4 * inf * 2.0 ** -24 * mag)[ok]).all())
    # 0 x inf of a dropped position does not appear: out feature 3 of token 1 is finite unless a kept position met the inf
    if W[3, dropped] == 0 and not bool(torch.isinf(W[3]).any() | torch.isnan(W[3]).any()):
        assert bool(torch.isfinite(got[1, 3])), "an inf of X met a dropped position of W"
    # a token row of NaNs beyond `tokens` poisoned nothing: rows without NaN / inf inputs are finite where W's row is
    clean_t = 3
    clean_o = [o for o in range(out) if o not in (7, 9)]
    assert bool(torch.isfinite(got[clean_t, clean_o]).all())


# ------------------------------------------------------------------------------------------------ hipGraph
@pytest.mark.parametrize("tokens", [8, 200])
def test_hipgraph_replay_gives_the_eager_bits(gpu, tokens):
    pkg = gpu
    out, inf, bf = 512, 512, False
    W = pruned_weight(pkg, out, inf, bf, 81)
    blob = compress(pkg, W, out, inf)
    X = rand((tokens, inf), bf, 82)
    bias = (torch.rand(out, device=DEV) * 2 - 1).float()
    ep = pkg.Epilogue(bias=bias, act="relu")
    eager = torch.full((tokens, out), 9.0, dtype=DT[bf], device=DEV)
    pkg.linear24(blob, X, eager, tokens, out, inf, epilogue=ep)
    torch.cuda.synchronize()
    Y = torch.full((tokens, out), 5.0, dtype=DT[bf], device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pkg.linear24(blob, X, Y, tokens, out, inf, epilogue=ep)
    Y.fill_(5.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(Y), bits(eager))


# ------------------------------------------------------------------------------------------------ the C++ headers
def test_linear_through_the_cpp_headers(gpu):
    """spmma_plan_t<T>::linear (include/sparsify.me/spmma.hxx), with and without an epilogue, fp16 and bfloat16: the binary checks
    its results against the three-call route through the same headers and writes Y of one case, compared here with the Python result."""
    pkg = gpu
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "linear24.mk"], check=True, capture_output=True)
    dump = os.path.join(ROOT, "tests", "cpp", "bin", "linear24_dump.bin")
    if os.path.exists(dump):
        os.remove(dump)
    res = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "linear24_headers"), dump], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "linear24_headers ok" in res.stdout
    # the dumped case: tokens, out, in as int64, then W (pruned, fp16), X, Y
    raw = np.fromfile(dump, dtype=np.uint8)
    tokens, out, inf = (int(v) for v in raw[:24].view(np.int64))
    body = raw[24:].view(np.uint16)
    Wn, Xn, Yn = body[:out * inf], body[out * inf:out * inf + tokens * inf], body[out * inf + tokens * inf:]
    assert Yn.size == tokens * out
    W = torch.from_numpy(Wn.astype(np.int16)).view(torch.float16).reshape(out, inf).to(DEV)
    X = torch.from_numpy(Xn.astype(np.int16)).view(torch.float16).reshape(tokens, inf).to(DEV)
    blob = compress(pkg, W, out, inf)
    Y = torch.empty(tokens, out, dtype=torch.float16, device=DEV)
    pkg.linear24(blob, X, Y, tokens, out, inf)
    torch.cuda.synchronize()
    assert np.array_equal(Y.cpu().view(torch.int16).numpy().view(np.uint16).ravel(), Yn)
