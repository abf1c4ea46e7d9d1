"""sm_moe_combine_{f16,bf16} on the device, and the whole MoE block end to end.

The combine is a fixed fp32 expression with one rounding, so every comparison is bit for bit against the numpy restatement below
(float32 multiply, float32 add, j ascending, then one rounding to nearest even; NaN compared as NaN): top_k 1 / 2 / 3 / 8, weights NULL
and given, R NULL / R == out / a separate R, dropped pairs and pairs with pos >= rows_p, a token with every pair dropped, odd hidden,
ldp and ldo beyond hidden with NaN in the padding, a sentinel-guarded out, NaN / inf / -0 inputs, and operands on which an fma and the
multiply-then-add differ in the rounded result (the no-contraction rule).  Both forms are asserted through sm_moe_combine_form.

End to end: route -> gated gathered layer -> down projection -> combine at 8 experts, top-2, in 64 -> 192 -> hidden 44, bit for bit
against torch.sort + index_select + the existing grouped calls + the numpy combine; once in a captured graph under two routings."""
import numpy as np
import pytest
import torch
from linear24_testlib import DEV, DT, SENTINEL, TYPES, mask24

pytestmark = pytest.mark.gpu

GUARD = 3


def bits(t):
    return t.contiguous().view(torch.int16)


def to_type(a32, ty):
    """fp32 numpy -> the 16-bit type, one rounding to nearest even (numpy's for fp16, torch's for bf16)"""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if ty == "f16":
        with np.errstate(over="ignore"):
            return torch.from_numpy(a32.astype(np.float16))
    return torch.from_numpy(a32).to(torch.bfloat16)


def combine_ref(Yp, pair_pos, weights, R, tokens, top_k, hidden, rows_p):
    """fp32 to the operation: s = R or +0; q = w * y one float32 multiply, s = s + q one float32 add, j ascending; the fp32 sums"""
    Yp = np.asarray(Yp, dtype=np.float32)
    s = np.zeros((tokens, hidden), dtype=np.float32) if R is None else np.asarray(R, dtype=np.float32)[:, :hidden].copy()
    pos = np.asarray(pair_pos).reshape(tokens, top_k)
    w = None if weights is None else np.asarray(weights, dtype=np.float32).reshape(tokens, top_k)
    with np.errstate(all="ignore"):
        for j in range(top_k):
            ok = (pos[:, j] >= 0) & (pos[:, j] < rows_p)
            y = Yp[np.where(ok, pos[:, j], 0)][:, :hidden]
            q = y if w is None else (w[:, j:j + 1] * y).astype(np.float32)
            s = np.where(ok[:, None], (s + q).astype(np.float32), s)
    return s


def assert_same(got, want, what):
    """bit for bit, NaN compared as NaN"""
    g, w = got.cpu(), want.cpu()
    gn, wn = torch.isnan(g), torch.isnan(w)
    bad = torch.nonzero((gn != wn) | (~gn & (bits(g) != bits(w))))
    assert bad.numel() == 0, f"{what}: first mismatch at {bad[0].tolist()}: {g[tuple(bad[0])].item()} for {w[tuple(bad[0])].item()}, {len(bad)} of {g.numel()}"


def run_case(pkg, ty, rng, tokens, top_k, hidden, rows_p, weights, rmode, pad, form, Yp=None, pos=None, w=None, R=None):
    """rmode: None / "inplace" / "separate"; pad: extra elements of ldp and ldo (NaN inside)"""
    Pn = tokens * top_k
    ldp, ldo = hidden + pad, hidden + pad
    Yp = rng.uniform(-2, 2, (rows_p, hidden)) if Yp is None else Yp
    if pos is None:
        pos = rng.integers(-2, rows_p + 3, Pn)
        pos[:top_k] = np.array([-1, rows_p, -5, rows_p + 7, -1, -1, rows_p, -2])[:top_k]     # token 0: every pair dropped or out of range
    w = (rng.uniform(-1.5, 1.5, Pn).astype(np.float32) if weights else None) if w is None else w
    R = (rng.uniform(-2, 2, (tokens, hidden)) if rmode else None) if R is None else R
    Yd = torch.full((rows_p, ldp), float("nan"), dtype=DT[ty], device=DEV)
    Yd[:, :hidden] = to_type(Yp, ty).to(DEV)
    Ob = torch.full((tokens + 2 * GUARD, ldo), SENTINEL, dtype=DT[ty], device=DEV)
    O = Ob[GUARD:GUARD + tokens]
    Rd = None
    if rmode == "inplace":
        O[:, :hidden] = to_type(R, ty).to(DEV)
        Rd = O
    elif rmode == "separate":
        Rd = torch.full((tokens, ldo), float("nan"), dtype=DT[ty], device=DEV)
        Rd[:, :hidden] = to_type(R, ty).to(DEV)
    assert pkg.moe_combine_form(Yd, Rd, O, hidden, ldp, ldo) == form
    pd = torch.from_numpy(np.asarray(pos, dtype=np.int32)).to(DEV)
    wd = torch.from_numpy(w).to(DEV) if w is not None else None
    pkg.moe_combine(Yd, pd, O, tokens, top_k, hidden, rows_p, weights=wd, residual=Rd, ldp=ldp, ldo=ldo)
    torch.cuda.synchronize()
    assert bool((Ob[:GUARD] == SENTINEL).all()) and bool((Ob[GUARD + tokens:] == SENTINEL).all()), "a guard row of out was written"
    assert bool((O[:, hidden:] == SENTINEL).all()), "columns at or beyond hidden were written"
    s = combine_ref(to_type(Yp, ty).float().numpy(), pos, w, None if R is None else to_type(R, ty).float().numpy(), tokens, top_k, hidden, rows_p)
    want = to_type(s, ty)
    assert_same(O[:, :hidden], want, f"{ty} top_k {top_k} {form}")
    if top_k <= 8 and pos is not None and all(not (0 <= p < rows_p) for p in np.asarray(pos)[:top_k]):
        row0 = to_type(R, ty)[0] if R is not None else torch.zeros(hidden, dtype=DT[ty])
        assert torch.equal(bits(O[0, :hidden].cpu()), bits(row0)), "a token with every pair dropped gives R, or +0"
    return O, want


CASES = [(1, False, None), (1, True, "separate"), (2, True, None), (2, False, "inplace"), (3, True, "inplace"), (3, False, "separate"), (8, True, "separate"),
         (8, True, "inplace"), (8, False, None)]


@pytest.mark.parametrize("top_k,weights,rmode", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("ty", TYPES)
def test_vec_form(gpu, ty, top_k, weights, rmode):
    """hidden 72, ldp = ldo = 80: 16-byte pieces; 300 tokens x 9 pieces: more than one workgroup"""
    run_case(gpu, ty, np.random.default_rng(3000 + top_k), 300, top_k, 72, 500, weights, rmode, 8, "vec")


@pytest.mark.parametrize("top_k,weights,rmode", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("ty", TYPES)
def test_scalar_form_odd_hidden(gpu, ty, top_k, weights, rmode):
    run_case(gpu, ty, np.random.default_rng(3100 + top_k), 37, top_k, 45, 90, weights, rmode, 3, "scalar")


@pytest.mark.parametrize("ty", TYPES)
def test_scalar_form_by_alignment_alone(gpu, ty):
    """hidden % 8 == 0 but ldp % 8 != 0: per-element accesses, the same values"""
    run_case(gpu, ty, np.random.default_rng(3200), 20, 2, 64, 50, True, "separate", 4, "scalar")


@pytest.mark.parametrize("form,hidden,pad", [("vec", 64, 8), ("scalar", 45, 1)])
@pytest.mark.parametrize("ty", TYPES)
def test_nan_inf_and_negative_zero(gpu, ty, form, hidden, pad):
    rng = np.random.default_rng(3300)
    tokens, top_k, rows_p = 24, 3, 40
    Yp = rng.uniform(-2, 2, (rows_p, hidden))
    Yp[3, 5], Yp[4, 6], Yp[5, 7], Yp[6, :] = np.nan, np.inf, -np.inf, -0.0
    R = rng.uniform(-2, 2, (tokens, hidden))
    R[2, 1], R[7, :] = np.nan, -0.0
    pos = rng.integers(0, rows_p, tokens * top_k)
    pos[0:3] = [3, 4, 5]
    pos[3:6] = [4, 5, 9]          # inf + -inf in column-disjoint places, and inf - inf nowhere: kept simple
    pos[21:24] = [6, -1, -1]      # token 7: R = -0, y = -0: w * (-0) keeps or flips the sign with w's
    w = rng.uniform(0.5, 1.5, tokens * top_k).astype(np.float32)
    w[21] = -1.0
    O, want = run_case(gpu, ty, rng, tokens, top_k, hidden, rows_p, True, "separate", pad, form, Yp=Yp, pos=pos, w=w, R=R)
    assert bool(torch.isnan(want[0, 5])) and bool(torch.isinf(want[0, 6])) and bool(torch.isnan(want[2, 1]))
    # token 7: -0 + (-1 * -0 = +0) = +0 under round to nearest
    assert bits(O[7, :hidden].cpu()).tolist() == [0] * hidden
    # without weights and with R = -0: -0 + -0 = -0
    pos2 = np.full(tokens * top_k, -1)
    pos2[21] = 6
    O, _ = run_case(gpu, ty, rng, tokens, top_k, hidden, rows_p, False, "separate", pad, form, Yp=Yp, pos=pos2, R=R)
    assert bits(O[7, :hidden].cpu()).tolist() == [-32768] * hidden


def fma_witness(ty):
    """s, w, y with  round(fl32(s + fl32(w * y)))  !=  round(fl32(s + w * y)):  s = 1, the exact product just above a + 2^-24 with a half
    an ulp of the output type at 1 -- the product rounds to a + 2^-24, the sum 1 + a + 2^-24 is a tie that fp32 rounds to the even
    1 + a, itself a tie that the output type rounds to the even 1; the fused sum lies above the fp32 tie, rounds to 1 + a + 2^-23 and
    from there up to 1 + ulp.  All quantities fit 53 bits: float64 evaluates them exactly, np.float32() rounds once."""
    a = 2.0 ** -11 if ty == "f16" else 2.0 ** -8
    ulp = 2 * a
    for k in range(1, 200):
        y = float(to_type(np.array([1.0 + k * ulp]), ty).float()[0])
        w0 = np.float32((a + 2.0 ** -24) / y)
        for step in range(-3, 4):
            w = w0
            for _ in range(abs(step)):
                w = np.nextafter(w, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
            exact = float(w) * y                                   # <= 24 + 11 bits: exact in float64
            two_step = np.float32(np.float32(1.0) + np.float32(exact))
            fused = np.float32(1.0 + exact)                        # 1 + exact spans < 53 bits: exact, then one rounding
            r2, rf = to_type(np.array([two_step]), ty), to_type(np.array([fused]), ty)
            if bits(r2)[0] != bits(rf)[0]:
                return np.float32(w), y, float(r2.float()[0]), float(rf.float()[0])
    raise AssertionError("no witness found")


@pytest.mark.parametrize("form,hidden", [("vec", 8), ("scalar", 5)])
@pytest.mark.parametrize("ty", TYPES)
def test_multiply_and_add_are_not_contracted(gpu, ty, form, hidden):
    w, y, two_step, fused = fma_witness(ty)
    assert two_step != fused, "the chosen operands must differ under the two evaluations (verified here, on the CPU)"
    tokens, top_k, rows_p = 6, 1, 6
    Yp = np.full((rows_p, hidden), y)
    R = np.ones((tokens, hidden))
    O, want = run_case(gpu, ty, np.random.default_rng(3400), tokens, top_k, hidden, rows_p, True, "inplace", 0 if form == "vec" else 1, form, Yp=Yp,
                       pos=np.arange(tokens), w=np.full(tokens, w, dtype=np.float32), R=R)
    assert bool((want.float() == two_step).all()) and bool((O[:, :hidden].float().cpu() == two_step).all()), f"an fma would give {fused}"


# ------------------------------------------------------------------------------------------------ end to end
def compress(pkg, W):
    rows, inf = W.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 2, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24(W.contiguous(), rows, inf, inf, 1, rows * inf, blob)
    return blob


class Block:
    """8 experts, top-2: X[tokens][64] -> SwiGLU(gate/up) [P][192] -> down [P][44] -> combine [tokens][44]"""
    G, K, IN, MID, HID = 8, 2, 64, 192, 44

    def __init__(self, pkg, ty, tokens, seed):
        rng = np.random.default_rng(seed)
        self.pkg, self.ty, self.tokens, self.P = pkg, ty, tokens, tokens * self.K
        dt = DT[ty]
        w1 = np.where(mask24(rng, self.G * 2 * self.MID, self.IN), rng.uniform(-1, 1, (self.G * 2 * self.MID, self.IN)), 0.0)
        w2 = np.where(mask24(rng, self.G * self.HID, self.MID), rng.uniform(-0.5, 0.5, (self.G * self.HID, self.MID)), 0.0)
        self.b1 = compress(pkg, torch.from_numpy(w1).to(dt).to(DEV))
        self.b2 = compress(pkg, torch.from_numpy(w2).to(dt).to(DEV))
        self.X = torch.from_numpy(rng.uniform(-1, 1, (tokens, self.IN))).to(dt).to(DEV)
        self.R = torch.from_numpy(rng.uniform(-1, 1, (tokens, self.HID))).to(dt).to(DEV)
        P, G = self.P, self.G
        i32 = lambda n: torch.full((n,), -9, dtype=torch.int32, device=DEV)
        self.ids, self.w = i32(P), torch.zeros(P, dtype=torch.float32, device=DEV)
        self.off, self.st, self.sp, self.pp = i32(G + 1), i32(P), i32(P), i32(P)
        nb = pkg.moe_route_workspace_size(tokens, self.K, G)
        self.ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if nb else None
        self.Y1 = torch.zeros((P, self.MID), dtype=dt, device=DEV)
        self.Y2 = torch.zeros((P, self.HID), dtype=dt, device=DEV)
        self.out = torch.zeros((tokens, self.HID), dtype=dt, device=DEV)

    def new_block(self):
        pkg, G, K, P, T = self.pkg, self.G, self.K, self.P, self.tokens
        pkg.moe_route(self.ids, T, K, G, self.off, self.st, self.sp, self.pp, workspace=self.ws)
        pkg.linear24_grouped_glu(self.b1, self.X, self.Y1, self.off, G, P, self.MID, self.IN, act="silu", x_index=self.st, x_rows=T)
        pkg.linear24_grouped(self.b2, self.Y1, self.Y2, self.off, G, P, self.HID, self.MID)
        pkg.moe_combine(self.Y2, self.pp, self.out, T, K, self.HID, P, weights=self.w, residual=self.R)

    def parent_block(self):
        """torch.sort + bincount / cumsum + index_select + the existing grouped calls + the numpy combine"""
        pkg, G, K, P, T, dt = self.pkg, self.G, self.K, self.P, self.tokens, DT[self.ty]
        ids = self.ids.long()
        kept = (ids >= 0) & (ids < G)
        order = torch.sort(torch.where(kept, ids, torch.full_like(ids, G)), stable=True).indices[:int(kept.sum())]
        off = torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), torch.cumsum(torch.bincount(ids[kept], minlength=G), 0)]).int()
        V = order.numel()
        Xs = torch.zeros((P, self.IN), dtype=dt, device=DEV)
        Xs[:V] = self.X.index_select(0, order // K)
        Y1 = torch.zeros((P, self.MID), dtype=dt, device=DEV)
        Y2 = torch.zeros((P, self.HID), dtype=dt, device=DEV)
        pkg.linear24_grouped_glu(self.b1, Xs, Y1, off, G, P, self.MID, self.IN, act="silu")
        pkg.linear24_grouped(self.b2, Y1, Y2, off, G, P, self.HID, self.MID)
        torch.cuda.synchronize()
        pos = np.full(P, -1)
        pos[order.cpu().numpy()] = np.arange(V)
        s = combine_ref(Y2.float().cpu().numpy(), pos, self.w.cpu().numpy(), self.R.float().cpu().numpy(), T, K, self.HID, P)
        return to_type(s, self.ty)

    def set_routing(self, rng, drop=False):
        ids = np.argsort(rng.random((self.tokens, self.G)), axis=1)[:, :self.K].reshape(-1).astype(np.int32)
        if drop:
            ids[rng.random(self.P) < 0.2] = -1
            ids[rng.random(self.P) < 0.1] = self.G + 3
        self.ids.copy_(torch.from_numpy(ids).to(DEV))
        self.w.copy_(torch.from_numpy(rng.uniform(0.1, 0.9, self.P).astype(np.float32)).to(DEV))


@pytest.mark.parametrize("tokens", [150, 2100], ids=["single-route", "multi-route"])
@pytest.mark.parametrize("ty", TYPES)
def test_block_equals_the_composed_parent_route(gpu, ty, tokens):
    pkg = gpu
    blk = Block(pkg, ty, tokens, 3500 + tokens)
    assert pkg.moe_route_form(tokens, blk.K, blk.G) == ("single" if tokens == 150 else "multi")
    rng = np.random.default_rng(3600 + tokens)
    for drop in (False, True):
        blk.set_routing(rng, drop)
        blk.new_block()
        torch.cuda.synchronize()
        assert_same(blk.out, blk.parent_block(), f"block, drop={drop}")


def test_block_in_a_captured_graph_under_two_routings(gpu):
    """one stream, a chain of kernel nodes (no parallel branches); ids and weights then change in device memory only"""
    pkg = gpu
    blk = Block(pkg, "bf16", 150, 3700)
    rng = np.random.default_rng(3701)
    blk.set_routing(rng)
    blk.new_block()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        blk.new_block()
    outs = []
    for drop in (False, True):
        blk.set_routing(rng, drop)
        blk.out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        outs.append(blk.out.clone())
        assert_same(blk.out, blk.parent_block(), f"replay, drop={drop}")
    assert not torch.equal(bits(outs[0]), bits(outs[1]))
