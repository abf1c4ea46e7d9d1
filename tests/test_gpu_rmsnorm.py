"""sm_rmsnorm_{f16,bf16} on the device (-m gpu): residual add + RMSNorm with the 16-bit and / or the per-token fp8 output, in one launch.

Exact comparisons: res_out bit for bit with (H.float() + D.float()).to(dtype); Q and row_scale bit for bit with sm_quantize_rows_fp8_* run
on the device's own N (also when the fused call writes no N), NaN / inf rows, an all-zero row and both formats included; the call with D
against the call without D on the first call's res_out; a row alone against the same row inside 257 (and inside thousands).  On the
integer class (tests/rmsnorm_testlib.py: |h| <= 15, |gamma| <= 4 integers, so every partial sum of S is an exact fp32 integer in any order) the fp32
restatement is the definition and N is compared bit for bit with it, NaN as NaN, for several eps.  On general data N(0, sigma), sigma 0.01
/ 1 / 30, gamma ~ N(1, 0.3), N is held to the fp64 evaluation of the definition at the device's own h within half an ulp of the output
type at the larger of |ref| and |N| plus (hidden + 8) * 2^-24 * |ref| (hidden * 2^-24 bounds the fp32 sum in any order; 8 stands for the
division, add, square root, division, two multiplies and slack: an allowance, not a measurement).  Every case prints its worst error as a
share of that bound before it asserts.

Every call reads its operands at moved bases with pitches above `hidden` and NaN in the padding and writes outputs that sit between
sentinel words, in the padding of their rows too; nothing outside the outputs is written.  Every case asks sm_rmsnorm_form which form it
runs and runs twice (same bits).  Shapes: tokens 1, 3, 4, 5, 67, 257 (and the row counts at which a LANES wave takes more rows at
once); hidden 8, 64, 72, 128, 520, 2048, 4096, 8192, 16384 and both sides of RMSNORM_LANES_MAX_HIDDEN (the package constant); both types, both fp8 formats, 8-byte and per-byte stores into Q; every combination of
D / gamma / res_out / N / Q present or NULL; the allowed in-place aliasings."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import rmsnorm_testlib as rl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
TDT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
ALL = ("D", "gamma", "res", "N", "Q")


def form_of(pkg, hidden):
    return "lanes" if hidden <= pkg.RMSNORM_LANES_MAX_HIDDEN else "block"


class Norm:
    """One shape's operands.  use: which of D / gamma / res / N / Q the call gets; alias: "res=H", "N=D", "N=H" (with use deciding whether
    res_out is NULL) or "N=H,res=H"; qpad: Q's pitch above hidden (8: 8-byte stores, 3: an odd pitch and base, per-byte stores)."""

    def __init__(self, pkg, ty, tokens, hidden, fmt="e4m3", use=ALL, alias="", qpad=8):
        self.pkg, self.ty, self.tokens, self.hidden, self.fmt, self.use, self.alias = pkg, ty, tokens, hidden, fmt, set(use), alias
        op = lambda dtype, rows, cols, pitch, base, fill: rl.Operand(torch, dtype, rows, cols, pitch, base, fill, DEV)
        dt = DT[ty]
        self.H = op(dt, tokens, hidden, hidden + 8, 8, rl.NAN16[ty])
        self.D = op(dt, tokens, hidden, hidden + (8 if alias == "N=D" else 16), 16, rl.NAN16[ty])
        self.g = op(dt, 1, hidden, hidden, 8, rl.NAN16[ty])
        self.res = self.H if "res=H" in alias else op(dt, tokens, hidden, hidden + 8, 24, rl.SENT16)
        self.N = self.H if "N=H" in alias else self.D if alias == "N=D" else op(dt, tokens, hidden, hidden + 24, 8, rl.SENT16)
        self.Q = op(TDT[fmt], tokens, hidden, hidden + qpad, 8 if qpad % 8 == 0 else 5, rl.SENT8)
        self.rs = op(torch.float32, 1, tokens, tokens, 3, rl.SENT32)
        assert pkg.rmsnorm_form(hidden) == form_of(pkg, hidden)

    def has(self, name):
        return name in self.use

    def run(self, Hb, Db, gb, eps):
        """load, call, check that nothing but the outputs changed; returns the bits of the outputs the call has"""
        self.H.load(Hb)
        self.D.load(Db)
        self.g.load(gb[None, :])
        outs = [o for n, o in (("res", self.res), ("N", self.N), ("Q", self.Q), ("Q", self.rs)) if self.has(n)]
        ins = [o for o in (self.H, self.D, self.g) if all(o is not w for w in outs)]
        for o in outs:
            if o is not self.H and o is not self.D:
                o.raw.fill_(o.raw[0].item())                                 # back to the sentinel (element 0 is a guard word)
        before = [(o, o.snapshot()) for o in outs]
        whole = [(o, o.snapshot()) for o in ins]
        self.pkg.rmsnorm(self.H.view, delta=self.D.view if self.has("D") else None, gamma=self.g.view[0] if self.has("gamma") else None, eps=eps,
                         out=self.N.view if self.has("N") else None, res_out=self.res.view if self.has("res") else None,
                         fp8=(self.Q.view, self.rs.view[0]) if self.has("Q") else None)
        torch.cuda.synchronize()
        for o, snap in before:
            assert o.outside_unchanged(snap), "an element outside an output (padding or guard) was written"
        for o, snap in whole:
            assert torch.equal(o.raw, snap), "an input was written"
        got = {}
        if self.has("res"):
            got["res"] = self.res.bits()
        if self.has("N"):
            got["N"] = self.N.bits()
        if self.has("Q"):
            got["Q"], got["rs"] = self.Q.bits(), self.rs.bits().view(np.uint32)[0]
        return got

    def twice(self, Hb, Db, gb, eps):
        a, b = self.run(Hb, Db, gb, eps), self.run(Hb, Db, gb, eps)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), "two runs on the same operands differ"
        return a


def torch_add(Hb, Db, ty):
    """(H.float() + D.float()).to(dtype) on the device, as bit patterns"""
    t = lambda b: torch.from_numpy(b.view(np.int16)).to(DEV).view(DT[ty])
    return (t(Hb).float() + t(Db).float()).to(DT[ty]).view(torch.int16).cpu().numpy().view(np.uint16)


def quantiser(pkg, n_bits, ty, fmt):
    """sm_quantize_rows_fp8_* on these N bits: (Q bytes, row_scale bits)"""
    tokens, hidden = n_bits.shape
    A = torch.from_numpy(np.ascontiguousarray(n_bits).view(np.int16)).to(DEV).view(DT[ty])
    Q = torch.zeros((tokens, hidden), dtype=torch.uint8, device=DEV).view(TDT[fmt])
    rs = torch.zeros(tokens, dtype=torch.float32, device=DEV)
    pkg.quantize_rows_fp8(A, Q, rs, tokens, hidden)
    torch.cuda.synchronize()
    return Q.view(torch.uint8).cpu().numpy(), rs.cpu().numpy().view(np.uint32)


def check_quant(pkg, got, n_bits, ty, fmt, label):
    q, s = quantiser(pkg, n_bits, ty, fmt)
    assert np.array_equal(got["rs"], s), f"{label}: row_scale differs from sm_quantize_rows_fp8 of N"
    bad = np.argwhere(got["Q"] != q)
    assert bad.size == 0, f"{label}: Q differs from sm_quantize_rows_fp8 of N, first at {bad[0].tolist()}: {got['Q'][tuple(bad[0])]:#x} for {q[tuple(bad[0])]:#x}"


# (tokens, hidden or "T" / "T+8", type, fp8 format, qpad): every tokens and hidden value of the docstring, both sides of the threshold in both types
INT_CASES = [(1, 8, "f16", "e4m3", 8), (3, 64, "bf16", "e5m2", 3), (257, 72, "f16", "e5m2", 8), (5, 128, "bf16", "e4m3", 3), (67, 520, "f16", "e4m3", 3),
             (4, 2048, "bf16", "e4m3", 8), (5, 4096, "f16", "e5m2", 8), (3, 8192, "bf16", "e5m2", 3), (4, 16384, "f16", "e4m3", 8), (7, 16384, "bf16", "e4m3", 8),
             (67, "T", "f16", "e4m3", 8), (5, "T", "bf16", "e5m2", 3), (5, "T+8", "f16", "e5m2", 3), (67, "T+8", "bf16", "e4m3", 8), (9, 1032, "bf16", "e4m3", 8),
             (9, 2560, "f16", "e4m3", 8), (9, 4608, "bf16", "e5m2", 8), (257, 8, "bf16", "e4m3", 8),
             # rows enough that a LANES wave takes four groups of rows at once (more than 2048 waves of 64 / 2^L rows), and both sides of that
             (20000, 8, "bf16", "e4m3", 8), (16500, 64, "f16", "e5m2", 3), (4200, 200, "f16", "e4m3", 8), (2048, "T", "bf16", "e4m3", 8), (2049, "T", "f16", "e5m2", 8)]


def hid(pkg, h):
    return {"T": pkg.RMSNORM_LANES_MAX_HIDDEN, "T+8": pkg.RMSNORM_LANES_MAX_HIDDEN + 8}.get(h, h)


@pytest.mark.parametrize("case", INT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_integer_class_bit_for_bit(gpu, case):
    tokens, hidden, ty, fmt, qpad = case
    hidden = hid(gpu, hidden)
    rng = np.random.default_rng(8000 + INT_CASES.index(case))
    Hb, Db, gb = rl.integer_rows(rng, tokens, hidden, ty)
    nm = Norm(gpu, ty, tokens, hidden, fmt, qpad=qpad)
    h = torch_add(Hb, Db, ty)
    assert rl.same_bits_nan_as_nan(h, rl.add_round(Hb, Db, ty), ty) and rl.integer_class(h, gb, ty)
    for eps in (0.0, 1e-6, 0.5):
        got = nm.twice(Hb, Db, gb, eps)
        assert np.array_equal(got["res"], h), "res_out differs from (H.float() + D.float()).to(dtype)"
        want = rl.norm32(h, gb, eps, ty)
        assert rl.same_bits_nan_as_nan(got["N"], want, ty), f"N differs from the definition at {np.argwhere(got['N'] != want)[:3].tolist()} (eps {eps})"
        check_quant(gpu, got, got["N"], ty, fmt, f"eps {eps}")
        if tokens >= 4 and eps == 0.0:
            n = rl.f32_of(got["N"], ty)
            assert np.isnan(n[tokens - 1]).all(), "an all-zero row with eps = 0 gives NaN"
            assert np.isnan(n[tokens - 2]).sum() == 1 and (n[tokens - 2][~np.isnan(n[tokens - 2])] == 0).all(), "an inf gives r = 0: zeros, NaN at the inf"


COMBOS = [c for c in itertools.product((False, True), repeat=5) if c[3] or c[4]]         # D, gamma, res, N, Q; N or Q


@pytest.mark.parametrize("ty,hidden,fmt", [("bf16", 72, "e4m3"), ("f16", "T+8", "e5m2"), ("bf16", "T", "e5m2")])
def test_every_combination_of_operands(gpu, ty, hidden, fmt):
    hidden = hid(gpu, hidden)
    tokens = 5
    rng = np.random.default_rng(8100 + hidden)
    Hb, Db, gb = rl.integer_rows(rng, tokens, hidden, ty)
    assert len(COMBOS) == 24
    for combo in COMBOS:
        use = [n for n, on in zip(ALL, combo) if on]
        nm = Norm(gpu, ty, tokens, hidden, fmt, use=use)
        got = nm.twice(Hb, Db, gb, 1e-6)
        h = torch_add(Hb, Db, ty) if "D" in use else Hb
        g = gb if "gamma" in use else None
        assert rl.integer_class(h, g, ty)
        want = rl.norm32(h, g, 1e-6, ty)
        assert set(got) == ({"res"} if "res" in use else set()) | ({"N"} if "N" in use else set()) | ({"Q", "rs"} if "Q" in use else set())
        if "res" in use:
            assert np.array_equal(got["res"], h), use
        if "N" in use:
            assert rl.same_bits_nan_as_nan(got["N"], want, ty), use
        if "Q" in use:                       # with N == NULL too: the quantiser on the N the sibling call (same operands, N given) wrote
            check_quant(gpu, got, got["N"] if "N" in use else Norm(gpu, ty, tokens, hidden, fmt, use=use + ["N"]).run(Hb, Db, gb, 1e-6)["N"], ty, fmt, str(use))


GEN_CASES = [(3, 8, "f16"), (5, 64, "bf16"), (67, 72, "bf16"), (257, 128, "f16"), (5, 520, "f16"), (4, 2048, "bf16"), (5, 4096, "bf16"), (3, 8192, "f16"),
             (3, 16384, "bf16"), (4, 16384, "f16"), (5, "T", "f16"), (4, "T", "bf16"), (5, "T+8", "bf16"), (4, "T+8", "f16"), (1, 4096, "f16"), (1, 520, "bf16")]


@pytest.mark.parametrize("case", GEN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_general_data_within_the_bound(gpu, case):
    tokens, hidden, ty = case
    hidden = hid(gpu, hidden)
    rng = np.random.default_rng(8200 + GEN_CASES.index(case))
    fmt = ("e4m3", "e5m2")[GEN_CASES.index(case) % 2]
    nm = Norm(gpu, ty, tokens, hidden, fmt, qpad=(8, 3)[(GEN_CASES.index(case) // 2) % 2])
    for sigma in (0.01, 1.0, 30.0):
        Hv, Dv = rng.normal(0.0, sigma, (tokens, hidden)), rng.normal(0.0, sigma, (tokens, hidden))
        if tokens >= 3:                      # a NaN and an inf among general data: their rows follow IEEE, the quantiser's bytes its rule
            Hv[tokens - 1, hidden // 3] = np.nan
            Dv[tokens - 2, hidden // 2] = -np.inf
        Hb, Db, gb = rl.bits_of(Hv, ty), rl.bits_of(Dv, ty), rl.bits_of(rng.normal(1.0, 0.3, hidden), ty)
        got = nm.twice(Hb, Db, gb, 1e-6)
        assert np.array_equal(got["res"], torch_add(Hb, Db, ty)), "res_out differs from (H.float() + D.float()).to(dtype)"
        ratio = rl.worst_ratio(got["N"], got["res"], gb, 1e-6, ty)
        print(f"margin rmsnorm general {ty} {tokens}x{hidden} sigma {sigma} {nm.pkg.rmsnorm_form(hidden)}: worst error {ratio:.3f} of the bound")
        assert ratio <= 1.0, f"error {ratio:.3f} of the bound (1/2 ulp + (hidden + 8) * 2^-24 |ref|)"
        check_quant(gpu, got, got["N"], ty, fmt, f"sigma {sigma}")


@pytest.mark.parametrize("ty,hidden", [("bf16", 72), ("f16", 520), ("bf16", "T"), ("f16", "T+8"), ("bf16", 8192)])
def test_with_D_equals_without_D_on_the_first_calls_res_out(gpu, ty, hidden):
    hidden = hid(gpu, hidden)
    tokens = 5
    rng = np.random.default_rng(8300 + hidden)
    Hb, Db, gb = (rl.bits_of(rng.normal(0.0, 1.0, s), ty) for s in ((tokens, hidden), (tokens, hidden), (hidden,)))
    first = Norm(gpu, ty, tokens, hidden).twice(Hb, Db, gb, 1e-5)
    second = Norm(gpu, ty, tokens, hidden, use=("gamma", "res", "N", "Q")).twice(first["res"], Db, gb, 1e-5)
    assert np.array_equal(second["res"], first["res"]), "without D the stream is unchanged"
    for k in ("N", "Q", "rs"):
        assert np.array_equal(first[k], second[k]), f"{k}: the fused call is not the composition of its parts"


@pytest.mark.parametrize("ty,hidden,fmt,rows", [("f16", 8, "e4m3", 257), ("bf16", 72, "e5m2", 257), ("f16", "T", "e4m3", 257), ("bf16", "T+8", "e4m3", 257),
                                                ("bf16", 4096, "e5m2", 257), ("bf16", 72, "e4m3", 8300), ("f16", "T", "e5m2", 2100)])
def test_a_row_alone_equals_the_row_among_many(gpu, ty, hidden, fmt, rows):
    """257 rows, and rows enough that the LANES form takes four groups of rows per wave where the single row takes one"""
    hidden = hid(gpu, hidden)
    rng = np.random.default_rng(8400 + hidden)
    Hb, Db, gb = (rl.bits_of(rng.normal(0.0, 1.0, s), ty) for s in ((rows, hidden), (rows, hidden), (hidden,)))
    many = Norm(gpu, ty, rows, hidden, fmt).twice(Hb, Db, gb, 1e-6)
    one = Norm(gpu, ty, 1, hidden, fmt)
    for t in (0, 130, rows - 2, rows - 1):
        got = one.twice(Hb[t:t + 1], Db[t:t + 1], gb, 1e-6)
        for k in ("res", "N", "Q"):
            assert np.array_equal(got[k][0], many[k][t]), f"{k} of row {t} depends on the rows that ride with it"
        assert got["rs"][0] == many["rs"][t]


@pytest.mark.parametrize("alias,use", [("res=H", ALL), ("N=D", ALL), ("N=D", ("D", "gamma", "N")), ("N=H", ("D", "gamma", "N", "Q")), ("N=H,res=H", ALL),
                                       ("N=H", ("gamma", "N"))])
@pytest.mark.parametrize("ty,hidden", [("bf16", 72), ("f16", "T"), ("bf16", "T+8")])
def test_allowed_in_place_aliasings(gpu, alias, use, ty, hidden):
    hidden = hid(gpu, hidden)
    tokens = 67
    rng = np.random.default_rng(8500 + hidden)
    Hb, Db, gb = rl.integer_rows(rng, tokens, hidden, ty)
    got = Norm(gpu, ty, tokens, hidden, use=use, alias=alias).twice(Hb, Db, gb, 1e-6)
    h = torch_add(Hb, Db, ty) if "D" in use else Hb
    want = rl.norm32(h, gb, 1e-6, ty)
    assert rl.same_bits_nan_as_nan(got["N"], want, ty), (alias, use)
    if "res" in use and "N=H" not in alias:
        assert np.array_equal(got["res"], h)
    if "Q" in use:
        check_quant(gpu, got, got["N"], ty, "e4m3", alias)


@pytest.mark.parametrize("ty,fmt", [("bf16", "e4m3"), ("f16", "e5m2")])
def test_hipgraph_add_norm_quant_then_linear24_fp8(gpu, ty, fmt):
    """add + norm + quant -> sm_linear24_fp8 captured once (one stream: a chain of kernel nodes) and replayed under two inputs; Y equals the
    unfused route bit for bit: torch add -> this call without Q -> sm_quantize_rows_fp8_* -> the layer"""
    pkg, tokens, hidden, out = gpu, 37, 256, 128
    dt, f8 = DT[ty], TDT[fmt]
    rng = np.random.default_rng(8600)
    t16 = lambda a: torch.from_numpy(rl.bits_of(a, ty).view(np.int16)).to(DEV).view(dt)
    W = t16(rng.normal(0.0, 0.05, (out, hidden)))
    blob = torch.zeros(pkg.compress24_size(out, hidden, 1, 1), dtype=torch.uint8, device=DEV)
    ws = torch.zeros(out, dtype=torch.float32, device=DEV)
    pkg.quantize_compress24_fp8(W, blob, ws, out, hidden, f8)
    gamma = t16(rng.normal(1.0, 0.3, hidden))
    H, D = torch.zeros((tokens, hidden), dtype=dt, device=DEV), torch.zeros((tokens, hidden), dtype=dt, device=DEV)
    res = torch.zeros_like(H)
    Q = torch.zeros((tokens, hidden), dtype=torch.uint8, device=DEV).view(f8)
    xs = torch.zeros(tokens, dtype=torch.float32, device=DEV)
    Y = torch.zeros((tokens, out), dtype=dt, device=DEV)

    def fused():
        pkg.rmsnorm(H, delta=D, gamma=gamma, eps=1e-6, res_out=res, fp8=(Q, xs))
        pkg.linear24_fp8(blob, Q, Y, tokens, out, hidden, w_dtype=f8, w_scale=ws, x_scale=xs)

    def unfused():
        h = (H.float() + D.float()).to(dt)
        n = pkg.rmsnorm(h, gamma=gamma, eps=1e-6)
        q2, xs2 = torch.zeros_like(Q.view(torch.uint8)).view(f8), torch.zeros_like(xs)
        pkg.quantize_rows_fp8(n, q2, xs2, tokens, hidden)
        y2 = torch.zeros_like(Y)
        pkg.linear24_fp8(blob, q2, y2, tokens, out, hidden, w_dtype=f8, w_scale=ws, x_scale=xs2)
        torch.cuda.synchronize()
        return h, y2

    inputs = [(t16(rng.normal(0.0, s, (tokens, hidden))), t16(rng.normal(0.0, s, (tokens, hidden)))) for s in (1.0, 0.05)]
    H.copy_(inputs[0][0])
    D.copy_(inputs[0][1])
    fused()                                          # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fused()
    for h_in, d_in in inputs + [inputs[0]]:
        H.copy_(h_in)
        D.copy_(d_in)
        for v in (res, Y):
            v.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        h, y2 = unfused()
        assert torch.equal(res.view(torch.int16), h.view(torch.int16)), "res_out of the replay differs from the torch add"
        assert torch.equal(Y.view(torch.int16), y2.view(torch.int16)), "the fused block differs from the unfused route"
        assert bool(torch.isfinite(Y.float()).all()) and float(Y.float().abs().max()) > 0


def test_cpp_header_mirror(gpu):
    """examples/bin/rmsnorm: sparsifyme::rmsnorm (add, gamma, fp8 output) -> sm_linear24_fp8 through the headers; the example checks res_out
    and the integer-class N on the host and the layer against the quantiser's route itself and exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "rmsnorm")
    assert os.path.exists(exe), "examples/bin/rmsnorm is missing: build() makes it"
    for argv in (["37", "256"], ["5", "4096", "e5m2"]):
        res = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.count(": yes") == 3 and "NO" not in res.stdout, res.stdout
