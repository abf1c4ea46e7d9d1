"""sm_linear24_fp8 on the device: Y[tokens][out] = act((alpha * w_scale[o]) * x_scale[t] * (X . W_2:4^T) + beta * R + bias), fp8 operands,
token-major in and out.  The reference is numpy fp64 on this file's own decode of the fp8 bytes.

* exact products (small integers, power-of-two scales) pin the K-contiguous X fragment, the 4-byte metadata pieces, the odd-plane tail
  and the untransposed store of both forms, every format pair and output type;
* every tile instantiation equals sm_spmma_fp8 + a transpose bit for bit, on padded X and a sentinel-guarded Y;
* scales and epilogues of the decode form and a tile form against fp64 within the bound of tests/test_gpu_fp8.py;
* the quantise -> layer pipeline end to end; NaN / inf, determinism, hipGraph replay.
Every test named for a form asks sm_linear24_fp8_form (at the device's compute-unit count) which form its shape runs."""
import os

import numpy as np
import pytest
import torch
from linear24_testlib import DEV, FMTS, NAN_BYTE, ODT, OUTS, PAIRS, ROUND, TDT, TINY, U_OPS, decode8, dev8, encode8, f32dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDT = {"f32": torch.int32, "f16": torch.int16, "bf16": torch.int16}
ACTS = [("none", 0.0), ("relu", 0.0), ("relu6", 6.0), ("leaky_relu", 0.1), ("hardswish", 0.0)]


def mask24(rng, out, inf):
    """two kept positions in every strip of four"""
    keep = np.argsort(rng.random((out, inf // 4, 4)), axis=2)[:, :, :2]
    m = np.zeros((out, inf // 4, 4), dtype=bool)
    np.put_along_axis(m, keep, True, axis=2)
    return m.reshape(out, inf)


def compress(pkg, wb, fmt):
    out, inf = wb.shape
    blob = torch.empty(pkg.compress24_size(out, inf, 1, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24_fp8(dev8(wb, fmt), out, inf, inf, 1, out * inf, blob)
    return blob


def bits(t):
    return t.contiguous().view(IDT[{v: k for k, v in ODT.items()}[t.dtype]])


def form_of(pkg, tokens, out, inf):
    return pkg.linear24_fp8_form(tokens, out, inf)


MARGINS = {}


def note_margin(form, ratio, what):
    if form not in MARGINS or ratio > MARGINS[form][0]:
        MARGINS[form] = (ratio, what)


@pytest.fixture(scope="module", autouse=True)
def _margin_report():
    yield
    if not MARGINS:
        return
    lines = ["sm_linear24_fp8: worst err / bound per form (bound: ROUND |ref| + (2 in + %d) 2^-24 S + TINY)" % U_OPS]
    lines += [f"{form:12s} {r:.4f}  {what}" for form, (r, what) in sorted(MARGINS.items())]
    print("\n".join(lines))
    d = os.environ.get("SM_PARITY_MARGINS_DIR")   # where a run that refreshes profiles/parity_margins_linear24_fp8.txt wants the file
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_margins_linear24_fp8.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------ 1. exact products
def int_operands(rng, tokens, out, inf, fw, fx, sparse_x=False):
    """W: two of every four kept, values in {-2, -1, 1, 2}; X: integers in [-2, 2] (sparse_x: one non-zero per 64 k)."""
    Wn = np.where(mask24(rng, out, inf), rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(out, inf)), 0.0)
    if sparse_x:
        Xn = np.zeros((tokens, inf // 64, 64))
        np.put_along_axis(Xn, rng.integers(0, 64, size=(tokens, inf // 64, 1)), rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(tokens, inf // 64, 1)), axis=2)
        Xn = Xn.reshape(tokens, inf)
    else:
        Xn = rng.integers(-2, 3, size=(tokens, inf)).astype(np.float64)
    wb, xb = encode8(Wn, fw), encode8(Xn, fx)
    assert np.array_equal(decode8(wb, fw), Wn) and np.array_equal(decode8(xb, fx), Xn)   # both formats hold them exactly
    return wb, xb, Xn @ Wn.T


def run_exact(pkg, rng, tokens, out, inf, fw, fx, o, scales, sparse_x=False):
    wb, xb, acc = int_operands(rng, tokens, out, inf, fw, fx, sparse_x)
    alpha = 0.5
    ws = rng.choice(np.array([0.5, 1.0, 2.0]), size=out) if scales else None
    xs = rng.choice(np.array([0.25, 1.0, 2.0]), size=tokens) if scales else None
    ref = alpha * acc * (ws[None, :] if scales else 1.0) * (xs[:, None] if scales else 1.0)
    want = torch.from_numpy(ref).to(ODT[o])
    if o != "bf16" or np.abs(acc).max() < 256:   # an integer below 2^8 (2^11, 2^24) times a power of two: held exactly
        assert np.array_equal(want.double().numpy(), ref)
    Y = torch.full((tokens, out), 9.0, dtype=ODT[o], device=DEV)
    pkg.linear24_fp8(compress(pkg, wb, fw), dev8(xb, fx), Y, tokens, out, inf, w_dtype=TDT[fw], alpha=alpha,
                     w_scale=f32dev(ws) if scales else None, x_scale=f32dev(xs) if scales else None)
    torch.cuda.synchronize()
    bad = np.argwhere(bits(Y).cpu().numpy() != bits(want).numpy())
    assert bad.size == 0, (f"tokens {tokens} out {out} in {inf}: first mismatch at (token, out) {bad[0]}: got {float(Y[tuple(bad[0])])}, "
                           f"want {float(want[tuple(bad[0])])}; {len(bad)} of {ref.size}")


@pytest.mark.parametrize("o", OUTS)
@pytest.mark.parametrize("fw,fx", PAIRS)
def test_integer_products_are_exact_in_both_forms(gpu, fw, fx, o):
    """|acc| <= 4 * in / 2 <= 768: every partial sum is an exact fp32 integer in any order, so Y is the fp64 product rounded once to the
    output type -- the product itself in fp32 and fp16, and in bf16 whenever |acc| < 2^8 (asserted where it holds).  in = 64, 192, 384:
    one plane, an odd plane count (the zero tail), an even one; odd out and out % 4 != 0 take the per-element store."""
    pkg = gpu
    rng = np.random.default_rng(1 + 10 * PAIRS.index((fw, fx)) + OUTS.index(o))
    seen = set()
    for inf in (64, 192, 384):
        for tokens in (1, 3, 16, 17, 64, 200):
            for out in (16, 100, 129, 130):
                seen.add(form_of(pkg, tokens, out, inf))
                run_exact(pkg, rng, tokens, out, inf, fw, fx, o, scales=inf != 192)
    assert seen == {"decode", "tile64"}


@pytest.mark.parametrize("fw,fx", PAIRS)
def test_decode_k_split_is_exact_on_integers(gpu, fw, fx):
    """in = 64 * 16 * 3: 24 stages over the decode form's 16 waves -- every wave multiplies, the second round is partial.  X has one
    non-zero per 64 k: |acc| <= 4 * 48 < 2^8, exact in every output type and any order."""
    pkg = gpu
    rng = np.random.default_rng(77 + PAIRS.index((fw, fx)))
    for i, (tokens, out) in enumerate(((3, 16), (16, 100), (1, 130))):
        assert form_of(pkg, tokens, out, 3072) == "decode"
        run_exact(pkg, rng, tokens, out, 3072, fw, fx, OUTS[i], scales=True, sparse_x=True)
    # an odd plane count in the split: the last stage of the last wave's share is the zero-tailed one
    assert form_of(pkg, 5, 16, 64 * 35) == "decode"
    run_exact(pkg, rng, 5, 16, 64 * 35, fw, fx, "f32", scales=False, sparse_x=True)


def test_decode_k_loop_goes_round_more_than_once(gpu):
    """A wave of the decode form requests four stages per turn of its loop, sixteen waves 64 stages: in = 64 * 269 is 135 stages -- a
    full second turn on reused registers, a third in which only waves 0 .. 6 have a stage, and the zero-tailed odd plane last; in =
    64 * 2 * 70 ends inside the second turn on an even plane count.  One non-zero per 64 k of X: |acc| <= 4 * 269 < 2^11, exact in fp32
    in any order."""
    pkg = gpu
    rng = np.random.default_rng(91)
    for k, (tokens, out, inf, (fw, fx)) in enumerate(((16, 40, 64 * 269, PAIRS[0]), (3, 17, 64 * 2 * 70, PAIRS[-1]))):
        assert form_of(pkg, tokens, out, inf) == "decode"
        run_exact(pkg, rng, tokens, out, inf, fw, fx, "f32", scales=bool(k), sparse_x=True)


# ------------------------------------------------------------------------------------------------ 2. tile form == the route
def rand_operands(rng, tokens, out, inf, fw, fx):
    wb = encode8(np.where(mask24(rng, out, inf), rng.uniform(-2, 2, (out, inf)), 0.0), fw)
    xb = encode8(rng.uniform(-2, 2, (tokens, inf)), fx)
    return wb, xb


def route(pkg, blob, xb, fx, fw, tokens, out, inf, o, alpha=1.0, beta=0.0, ws=None, Y0=None):
    """sm_spmma_fp8 with W as A (C[out][tokens], row_scale = w_scale), then a transpose.  xb: compact [tokens][in] bytes."""
    C = torch.full((out, tokens), 3.0, dtype=ODT[o], device=DEV) if Y0 is None else Y0.t().contiguous()
    pkg.spmma_fp8(blob, dev8(xb, fx), C, out, tokens, inf, alpha=alpha, beta=beta, row_scale=ws, a_dtype=TDT[fw])
    torch.cuda.synchronize()
    return C.t().contiguous()


TILE_SHAPES = [  # tokens, out, in, the form
    (17, 64, 64, "tile64"), (200, 328, 192, "tile64"), (77, 130, 256, "tile64"),
    (300, 16390, 128, "tile128"), (300, 16392, 192, "tile128"), (260, 8198, 128, "tile128x64"), (260, 8200, 192, "tile128x64"),
]


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
@pytest.mark.parametrize("fw,fx", PAIRS)
def test_tile_forms_equal_the_route_bit_for_bit(gpu, fw, fx, shape):
    """x_scale NULL, no epilogue struct, beta 0 and 0.5 in place; X with ldx > in and NaN bytes in the padding and behind the last token,
    Y with ldy > out, its slack columns and a tail row guarded by a sentinel."""
    pkg = gpu
    tokens, out, inf, want_form = shape
    assert form_of(pkg, tokens, out, inf) == want_form
    o = OUTS[(TILE_SHAPES.index(shape) + PAIRS.index((fw, fx))) % 3]
    rng = np.random.default_rng(200 + 10 * TILE_SHAPES.index(shape) + PAIRS.index((fw, fx)))
    wb, xb = rand_operands(rng, tokens, out, inf, fw, fx)
    blob = compress(pkg, wb, fw)
    ldx, ldy = inf + 16, out + 12
    xp = np.full((tokens + 1, ldx), NAN_BYTE[fx], dtype=np.uint8)
    xp[:tokens, :inf] = xb
    Xp = dev8(xp, fx)
    ws = f32dev(rng.uniform(0.5, 2.0, out))
    Y0 = torch.from_numpy(rng.uniform(-4, 4, (tokens, out)).astype(np.float32)).to(ODT[o]).to(DEV)
    for alpha, beta, scale in ((1.0, 0.0, None), (0.75, 0.5, ws)):
        Yp = torch.full((tokens + 1, ldy), 7.0, dtype=ODT[o], device=DEV)
        Yp[:tokens, :out] = Y0
        pkg.linear24_fp8(blob, Xp, Yp, tokens, out, inf, w_dtype=TDT[fw], ldx=ldx, ldy=ldy, alpha=alpha, beta=beta, w_scale=scale)
        ref = route(pkg, blob, xb, fx, fw, tokens, out, inf, o, alpha, beta, scale, Y0 if beta else None)
        assert torch.equal(bits(Yp[:tokens, :out]), bits(ref)), (alpha, beta)
        assert bool((Yp[:tokens, out:] == 7.0).all()) and bool((Yp[tokens] == 7.0).all()), "slack columns or the tail of Y were written"
    # a column slice whose start is one element off the piece alignment: the per-element store, same bits
    Yq = torch.full((tokens + 1, ldy), 7.0, dtype=ODT[o], device=DEV)
    pkg.linear24_fp8(blob, Xp, Yq.view(-1)[3:], tokens, out, inf, w_dtype=TDT[fw], ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    ref = route(pkg, blob, xb, fx, fw, tokens, out, inf, o)
    assert torch.equal(bits(Yq[:tokens, 3:3 + out]), bits(ref))
    assert bool((Yq[:tokens, :3] == 7.0).all()) and bool((Yq[:tokens, 3 + out:] == 7.0).all()) and bool((Yq[tokens, 3:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ 3. scales and epilogues vs fp64
def act64(x, act, arg):
    if act == "relu":
        return np.maximum(x, 0)
    if act == "relu6":
        return np.clip(x, 0, arg)
    if act == "leaky_relu":
        return np.where(x >= 0, x, arg * x)
    if act == "hardswish":
        return x * np.clip(x + 3, 0, 6) / 6
    return x


def bound_of(ref, S, inf, o):
    return ROUND[o] * np.abs(ref) + (2.0 * inf + U_OPS) * 2.0 ** -24 * S + TINY[o]


@pytest.mark.parametrize("o", OUTS)
@pytest.mark.parametrize("fw,fx", [("e4m3", "e4m3"), ("e5m2", "e4m3")])
@pytest.mark.parametrize("tokens,want_form", [(8, "decode"), (200, "tile64")])
def test_scales_and_epilogues_against_fp64(gpu, tokens, want_form, fw, fx, o):
    pkg = gpu
    out, inf = 328, 256
    assert form_of(pkg, tokens, out, inf) == want_form
    rng = np.random.default_rng(300 + tokens + 10 * FMTS.index(fw) + OUTS.index(o))
    wb, xb = rand_operands(rng, tokens, out, inf, fw, fx)
    blob, X = compress(pkg, wb, fw), dev8(xb, fx)
    W64, X64 = decode8(wb, fw), decode8(xb, fx)
    acc, mag = X64 @ W64.T, np.abs(X64) @ np.abs(W64).T
    ws, xs = rng.uniform(0.5, 2.0, out).astype(np.float32), rng.uniform(0.5, 2.0, tokens).astype(np.float32)
    dws, dxs = f32dev(ws), f32dev(xs)
    alpha, beta = 1.5, 0.5
    s = alpha * ws.astype(np.float64)[None, :] * xs.astype(np.float64)[:, None]
    R = torch.from_numpy(rng.uniform(-8, 8, (tokens, out)).astype(np.float32)).to(ODT[o]).to(DEV)
    R64 = R.double().cpu().numpy()
    b_out, b_tok = rng.uniform(-2, 2, out).astype(np.float32), rng.uniform(-2, 2, tokens).astype(np.float32)
    # the route on the same operands (fp32 out, no epilogue) inside its own bound: the inputs keep the reference itself honest
    C = torch.empty(out, tokens, dtype=torch.float32, device=DEV)
    pkg.spmma_fp8(blob, X, C, out, tokens, inf, alpha=alpha, row_scale=dws, a_dtype=TDT[fw])
    torch.cuda.synchronize()
    sr = alpha * ws.astype(np.float64)[None, :]
    rr = float((np.abs(C.t().double().cpu().numpy() - sr * acc) / (ROUND["f32"] * np.abs(sr * acc) + (2.0 * inf + 4.0) * 2.0 ** -24 * sr * mag + TINY["f32"])).max())
    print(f"route {fw} x {fx} tokens {tokens}: err / bound = {rr:.4f}")
    assert rr <= 1.0
    for act, arg in ACTS:
        for dim, bias in (("col", b_out), ("row", b_tok)):
            Y = torch.full((tokens, out), 9.0, dtype=ODT[o], device=DEV)
            pkg.linear24_fp8(blob, X, Y, tokens, out, inf, w_dtype=TDT[fw], alpha=alpha, beta=beta, w_scale=dws, x_scale=dxs,
                             epilogue=pkg.Epilogue(bias=f32dev(bias), bias_dim=dim, act=act, act_arg=arg, residual=R))
            torch.cuda.synchronize()
            bterm = bias.astype(np.float64)[None, :] if dim == "col" else bias.astype(np.float64)[:, None]
            ref = act64(s * acc + beta * R64 + bterm, act, arg)
            S = np.abs(s) * mag + np.abs(beta * R64) + np.abs(bterm)
            got = Y.double().cpu().numpy()
            ratio = float((np.abs(got - ref) / bound_of(ref, S, inf, o)).max())
            what = f"{want_form} {fw} x {fx} -> {o} tokens {tokens} {act} bias {dim}"
            print(f"{what}: err / bound = {ratio:.4f}")
            note_margin(want_form, ratio, what)
            assert np.isfinite(got).all() and ratio <= 1.0, what
    assert bool((R.double().cpu().numpy() == R64).all()), "the residual operand was written"


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("tokens", [8, 200])
def test_quantise_then_layer_end_to_end(gpu, tokens):
    """bf16 W and X in U(-1, 1): quantize_compress24_fp8 -> quantize_rows_fp8 -> linear24_fp8, against the fp64 product of the
    DEQUANTISED operands (the blob decompressed, the bytes decoded, times the scales the quantisers wrote)."""
    pkg = gpu
    out, inf, fmt, o = 328, 256, "e4m3", "bf16"
    g = torch.Generator(device=DEV).manual_seed(40 + tokens)
    W = (torch.rand(out, inf, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16)
    Xh = (torch.rand(tokens, inf, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16)
    blob = torch.empty(pkg.compress24_size(out, inf, 1, 1), dtype=torch.uint8, device=DEV)
    ws, xs = torch.empty(out, dtype=torch.float32, device=DEV), torch.empty(tokens, dtype=torch.float32, device=DEV)
    Q = torch.empty(tokens, inf, dtype=TDT[fmt], device=DEV)
    Y = torch.full((tokens, out), 9.0, dtype=ODT[o], device=DEV)
    pkg.quantize_compress24_fp8(W, blob, ws, out, inf, TDT[fmt])
    pkg.quantize_rows_fp8(Xh, Q, xs, tokens, inf)
    pkg.linear24_fp8(blob, Q, Y, tokens, out, inf, w_scale=ws, x_scale=xs)
    Wq = torch.empty(out, inf, dtype=TDT[fmt], device=DEV)
    pkg.decompress24_fp8(blob, out, inf, inf, 1, out * inf, Wq)
    torch.cuda.synchronize()
    W64, X64 = decode8(Wq.view(torch.uint8).cpu().numpy(), fmt), decode8(Q.view(torch.uint8).cpu().numpy(), fmt)
    s = ws.double().cpu().numpy()[None, :] * xs.double().cpu().numpy()[:, None]
    ref, S = s * (X64 @ W64.T), s * (np.abs(X64) @ np.abs(W64).T)
    got = Y.double().cpu().numpy()
    ratio = float((np.abs(got - ref) / bound_of(ref, S, inf, o)).max())
    form = form_of(pkg, tokens, out, inf)
    print(f"end to end tokens {tokens} ({form}): err / bound = {ratio:.4f}")
    note_margin(form, ratio, f"end to end {fmt} -> {o} tokens {tokens}")
    assert np.isfinite(got).all() and ratio <= 1.0


# ------------------------------------------------------------------------------------------------ 5. NaN / inf, determinism, graph
@pytest.mark.parametrize("fw,fx", [("e5m2", "e5m2"), ("e4m3", "e4m3"), ("e5m2", "e4m3")])
@pytest.mark.parametrize("tokens", [5, 40])
def test_nan_inf_propagate_as_in_the_route_and_runs_repeat(gpu, tokens, fw, fx):
    pkg = gpu
    out, inf, o = 96, 256, "f32"
    rng = np.random.default_rng(500 + tokens + FMTS.index(fw))
    wb, xb = rand_operands(rng, tokens, out, inf, fw, fx)
    kept = lambda row, n: int(np.flatnonzero(wb[row] & 0x7F)[n])
    wb[9, kept(9, 1)] = NAN_BYTE[fw]
    xb[0, 17] = NAN_BYTE[fx]
    if fw == "e5m2":
        wb[7, kept(7, 2)] = 0x7C                  # +inf at a kept position
    if fx == "e5m2":
        xb[1, int(np.flatnonzero((wb[3] & 0x7F) == 0)[0])] = 0x7C   # meets a dropped position of out feature 3, kept ones elsewhere
        xb[2, kept(5, 0)] = 0xFC                  # -inf
    blob = compress(pkg, wb, fw)
    xp = np.full((tokens + 8, inf), NAN_BYTE[fx], dtype=np.uint8)   # token rows beyond `tokens`: never read into a stored output
    xp[:tokens] = xb
    Y = torch.full((tokens + 8, out), 9.0, dtype=ODT[o], device=DEV)
    pkg.linear24_fp8(blob, dev8(xp, fx), Y, tokens, out, inf, w_dtype=TDT[fw])
    Y2 = torch.full((tokens + 8, out), 5.0, dtype=ODT[o], device=DEV)
    pkg.linear24_fp8(blob, dev8(xp, fx), Y2, tokens, out, inf, w_dtype=TDT[fw])
    ref = route(pkg, blob, xb, fx, fw, tokens, out, inf, o)
    got = Y[:tokens]
    assert bool((Y[tokens:] == 9.0).all())
    assert torch.equal(bits(got), bits(Y2[:tokens])), "two runs on the same inputs differ"
    assert torch.equal(got.isnan(), ref.isnan()) and bool(ref.isnan().any())
    assert torch.equal(got.isinf(), ref.isinf()) and torch.equal(got[ref.isinf()], ref[ref.isinf()])
    fin = ~ref.isnan()
    if form_of(pkg, tokens, out, inf) != "decode":   # a tile form: the route's bits
        assert torch.equal(bits(got)[fin], bits(ref)[fin])
    else:
        ok = (fin & ~ref.isinf()).cpu().numpy()
        clean = lambda a, f: np.nan_to_num(decode8(a, f), nan=0.0, posinf=0.0, neginf=0.0)
        mag = np.abs(clean(xb, fx)) @ np.abs(clean(wb, fw)).T
        g64, r64 = got.double().cpu().numpy()[ok], ref.double().cpu().numpy()[ok]
        assert bool((np.abs(g64 - r64) <= 2 * ROUND[o] * np.abs(r64) + 4.0 * inf * 2.0 ** -24 * mag[ok]).all())
    # rows and columns without a NaN / inf input are finite: the NaN rows behind the last token and the NaN padding poisoned nothing
    clean_o = [c for c in range(out) if c not in (7, 9)]
    assert bool(torch.isfinite(got[3, clean_o]).all())
    if fx == "e5m2":   # 0 x inf of a dropped position does not appear: out feature 3 has no non-finite weight
        assert bool(torch.isfinite(got[1, 3])), "an inf of X met a dropped position of W"


@pytest.mark.parametrize("tokens", [8, 200])
def test_hipgraph_replay_gives_the_eager_bits(gpu, tokens):
    pkg = gpu
    out, inf, fw, fx, o = 512, 512, "e4m3", "e4m3", "bf16"
    rng = np.random.default_rng(600 + tokens)
    wb, xb = rand_operands(rng, tokens, out, inf, fw, fx)
    blob, X = compress(pkg, wb, fw), dev8(xb, fx)
    ws, xs = f32dev(rng.uniform(0.5, 2.0, out)), f32dev(rng.uniform(0.5, 2.0, tokens))
    ep = pkg.Epilogue(bias=f32dev(rng.uniform(-1, 1, out)), act="relu")
    eager = torch.full((tokens, out), 9.0, dtype=ODT[o], device=DEV)
    pkg.linear24_fp8(blob, X, eager, tokens, out, inf, w_scale=ws, x_scale=xs, epilogue=ep)
    torch.cuda.synchronize()
    Y = torch.full((tokens, out), 5.0, dtype=ODT[o], device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):      # one stream, one kernel node: no parallel branches
        pkg.linear24_fp8(blob, X, Y, tokens, out, inf, w_scale=ws, x_scale=xs, epilogue=ep)
    Y.fill_(5.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(Y), bits(eager))
