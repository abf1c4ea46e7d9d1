"""sm_linear24_grouped_fp8 and sm_linear24_grouped_glu_fp8 on the device: `groups` experts of one shape, tokens sorted by expert, the
per-expert offsets read from device memory, one launch.

1. bit equality per group with sm_linear24_fp8 / sm_linear24_glu_fp8 on that slice of X and expert g's blob compressed alone, in every
   tile instantiation, plain and gated, with both scales (w_scale expert-major, x_scale in Y's rows): group sizes 0 (first, middle,
   last), 1, BN - 1, BN, BN + 1 and several tiles, off[0] > 0 and off[groups] < tokens, odd and packed widths, in = 64 (one plane: an
   odd plane count, shorter than the ring), 128, 192, 320; every format pair and output type on one shape; the epilogues;
2. integer operands: the fp64 product rounded once, per group;
3. offsets out of contract: nothing outside the `tokens` rows is touched, every row outside the overlap is exact;
4. NaN reaches exactly the rows it feeds; two runs and hipGraph replays under changed offsets give the eager bits.
Every call runs on X with ldx > in, NaN bytes in the padding and NaN guard rows before and behind the tokens inside the same
allocation, and on a sentinel-filled Y with ldy > out and guard rows of its own.  Every case asks the form query -- with the device's
compute units, as the fp8 layers do -- which form it runs."""
import numpy as np
import pytest
import torch
from linear24_testlib import (BN, CID, DEV, GUARD, NAN_BYTE, ODT, OUTS, PAIRS, SENTINEL, TDT, TID, TIGHT, dev8, encode8, f32dev, layout,
                              mask24, ranges, sizes, tight_layout)

pytestmark = pytest.mark.gpu

IDT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


# form, out of the plain case (odd: per-element stores; % 4 == 0: packed), hidden of the gated one, in.  The sizes() of a 64-token tile are
# 401 tokens in 7 tiles, mean 51; those of a 128-token tile 785 tokens in 7 tiles, mean 99: 37 tile rows (> 4608 blob rows) reach 256 workgroups
CASES = [("tile64", 77, 41, 64), ("tile64", 84, 44, 192), ("tile128x64", 4613, 2307, 64), ("tile128x64", 4612, 2308, 320),
         ("tile128", 4613, 2307, 128), ("tile128", 4612, 2308, 192)]


def bits(t):
    return t.contiguous().view(IDT[t.dtype])


def i32dev(a):
    return torch.tensor([int(v) for v in a], dtype=torch.int32, device=DEV)


def compress(pkg, W8):
    rows, inf = W8.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 1, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24_fp8(W8.contiguous(), rows, inf, inf, 1, rows * inf, blob)
    return blob


class Problem:
    """groups experts W[g][rows][in] (2:4) and X[tokens][in] as fp8 bytes in guarded, padded buffers; the stacked blob and each expert's
    own; w_scale (groups * rows, expert-major) and x_scale (tokens, Y's rows)"""

    def __init__(self, pkg, rng, fw, fx, o, groups, rows, inf, tokens, W=None, X=None):
        self.pkg, self.fw, self.fx, self.o, self.groups, self.rows, self.inf, self.tokens = pkg, fw, fx, o, groups, rows, inf, tokens
        Wn = np.where(mask24(rng, groups * rows, inf), rng.uniform(-2, 2, (groups * rows, inf)), 0.0) if W is None else W
        Xn = rng.uniform(-2, 2, (tokens, inf)) if X is None else X
        self.W8 = dev8(encode8(Wn, fw), fw)
        self.blob = compress(pkg, self.W8)
        self.own = [compress(pkg, self.W8[g * rows:(g + 1) * rows]) for g in range(groups)]
        self.ldx = inf + 16
        xb = np.full((tokens + 2 * GUARD, self.ldx), NAN_BYTE[fx], dtype=np.uint8)
        xb[GUARD:GUARD + tokens, :inf] = encode8(Xn, fx)
        self.Xbuf = dev8(xb, fx)
        self.X = self.Xbuf[GUARD:GUARD + tokens]
        self.ws = f32dev(rng.uniform(0.5, 2.0, groups * rows))
        self.xs = f32dev(rng.uniform(0.5, 2.0, tokens))
        self.kw = dict(w_dtype=TDT[fw], ldx=self.ldx)

    def ybuf(self, width, fill=None):
        ldy = width + 12
        Yb = torch.full((self.tokens + 2 * GUARD, ldy), SENTINEL, dtype=ODT[self.o], device=DEV)
        if fill is not None:
            Yb[GUARD:GUARD + self.tokens, :width] = fill
        self.before = Yb.clone()
        return Yb, ldy

    def slice_x(self, lo, hi):
        """rows lo .. hi-1 of X (and of x_scale) padded to >= 17 tokens: the plain call then runs a tile form"""
        n = max(hi - lo, 17)
        Xs = torch.zeros((n, self.ldx), dtype=torch.uint8, device=DEV)
        Xs[:hi - lo] = self.X[lo:hi].view(torch.uint8)
        Xs[:, self.inf:] = NAN_BYTE[self.fx]
        xs = torch.ones(n, dtype=torch.float32, device=DEV)
        xs[:hi - lo] = self.xs[lo:hi]
        return Xs.view(TDT[self.fx]), xs, n


def check_untouched(pr, Yb, width, owned):
    """guard rows, slack columns and rows no group owns keep the bits they had (the sentinel's; a residual's where Y was one)"""
    free = torch.ones(pr.tokens + 2 * GUARD, dtype=torch.bool, device=DEV)
    for lo, hi in owned:
        free[GUARD + lo:GUARD + hi] = False
    assert torch.equal(bits(Yb[free]), bits(pr.before[free])), "a row no group owns, or a guard row, was written"
    assert bool((Yb[:, width:] == SENTINEL).all()), "columns at or beyond the width of Y were written"


def assert_bits(got, ref, what):
    bad = torch.nonzero(bits(got) != bits(ref))
    assert bad.numel() == 0, f"{what}: first mismatch at (token, feature) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


def run_plain(pr, off, out, scales=True, epi=None, alpha=1.0, beta=0.0, fill=None):
    Yb, ldy = pr.ybuf(out, fill)
    Y = Yb[GUARD:GUARD + pr.tokens]
    pr.pkg.linear24_grouped_fp8(pr.blob, pr.X, Y, i32dev(off), pr.groups, pr.tokens, out, pr.inf, ldy=ldy, alpha=alpha, beta=beta,
                                w_scale=pr.ws if scales else None, x_scale=pr.xs if scales else None, epilogue=epi, **pr.kw)
    torch.cuda.synchronize()
    return Yb, Y


def run_glu(pr, off, hidden, act="silu", scales=True, bias=None):
    Yb, ldy = pr.ybuf(hidden)
    Y = Yb[GUARD:GUARD + pr.tokens]
    pr.pkg.linear24_grouped_glu_fp8(pr.blob, pr.X, Y, i32dev(off), pr.groups, pr.tokens, hidden, pr.inf, act=act, ldy=ldy,
                                    w_scale=pr.ws if scales else None, x_scale=pr.xs if scales else None, bias=bias, **pr.kw)
    torch.cuda.synchronize()
    return Yb, Y


def ref_plain(pr, g, lo, hi, out, scales=True, Y0=None, **kw):
    Xs, xs, n = pr.slice_x(lo, hi)
    assert pr.pkg.linear24_fp8_form(n, out, pr.inf).startswith("tile")
    Yr = torch.full((n, out), SENTINEL, dtype=ODT[pr.o], device=DEV) if Y0 is None else Y0
    pr.pkg.linear24_fp8(pr.own[g], Xs, Yr, n, out, pr.inf, w_scale=pr.ws[g * out:(g + 1) * out] if scales else None, x_scale=xs if scales else None,
                        **pr.kw, **kw)
    torch.cuda.synchronize()
    return Yr[:hi - lo]


def ref_glu(pr, g, lo, hi, hidden, scales=True, **kw):
    Xs, xs, n = pr.slice_x(lo, hi)
    assert pr.pkg.linear24_glu_form(n, hidden, pr.inf).startswith("tile")
    Yr = torch.full((n, hidden), SENTINEL, dtype=ODT[pr.o], device=DEV)
    pr.pkg.linear24_glu_fp8(pr.own[g], Xs, Yr, n, hidden, pr.inf, w_scale=pr.ws[g * 2 * hidden:(g + 1) * 2 * hidden] if scales else None,
                            x_scale=xs if scales else None, **pr.kw, **kw)
    torch.cuda.synchronize()
    return Yr[:hi - lo]


def compare_groups(pr, Y, off, width, ref):
    for g, (lo, hi) in enumerate(ranges(off, pr.tokens)):
        if hi > lo:
            assert_bits(Y[lo:hi, :width], ref(g, lo, hi), f"group {g} [{lo}, {hi})")


# ------------------------------------------------------------------------------------------------ 1. every tile instantiation
@pytest.mark.parametrize("case", CASES, ids=CID)
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_groups_equal_the_plain_layers_bit_for_bit(gpu, gated, case):
    pkg = gpu
    form, out, hidden, inf = case
    i = CASES.index(case)
    (fw, fx), o = PAIRS[(i + gated) % 4], OUTS[(i + 2 * gated) % 3]
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    rows = 2 * hidden if gated else out
    width = hidden if gated else out
    assert pkg.linear24_grouped_form(tokens, G, rows, inf) == form
    rng = np.random.default_rng(2000 + 2 * i + gated)
    pr = Problem(pkg, rng, fw, fx, o, G, rows, inf, tokens)
    if gated:
        bias = f32dev(rng.uniform(-1, 1, G * rows))
        run = lambda: run_glu(pr, off, hidden, "silu", bias=bias)
        ref = lambda g, lo, hi: ref_glu(pr, g, lo, hi, hidden, act="silu", bias=bias[g * rows:(g + 1) * rows])
    else:
        run = lambda: run_plain(pr, off, out)
        ref = lambda g, lo, hi: ref_plain(pr, g, lo, hi, out)
    Yb, Y = run()
    check_untouched(pr, Yb, width, ranges(off, tokens))
    compare_groups(pr, Y, off, width, ref)
    again, _ = run()
    assert torch.equal(bits(Yb), bits(again)), "two runs on the same inputs differ"


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_every_format_pair_and_output_type(gpu, gated):
    """One shape, both scales: 4 format pairs x 3 output types."""
    pkg = gpu
    rows, inf = (82, 192) if gated else (77, 192)
    width = rows // 2 if gated else rows
    counts = [0, 66, 1, 64]
    off, tokens = layout(counts, head=1, tail=2)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, rows, inf) == "tile64"
    for k, ((fw, fx), o) in enumerate((p, o) for p in PAIRS for o in OUTS):
        pr = Problem(pkg, np.random.default_rng(2100 + k), fw, fx, o, G, rows, inf, tokens)
        if gated:
            Yb, Y = run_glu(pr, off, width, "relu")
            ref = lambda g, lo, hi: ref_glu(pr, g, lo, hi, width, act="relu")
        else:
            Yb, Y = run_plain(pr, off, width, alpha=0.75)
            ref = lambda g, lo, hi: ref_plain(pr, g, lo, hi, width, alpha=0.75)
        check_untouched(pr, Yb, width, ranges(off, tokens))
        compare_groups(pr, Y, off, width, ref)


# ------------------------------------------------------------------------------------------------ 1b. every slot real, T % 8 != 0
# Routings that ATTAIN the slot bound min(tokens, ceil(tokens / 64) + groups - 1) -- no block of the grid is spare -- with a real-tile
# count T = tiles_m * slots that is no multiple of 8 (the XCD remap's unit): one group; one token per group; counts = 1 mod 64.
# (counts, out of the plain case, hidden of the gated one): tiles_m = ceil(out / 64) = ceil(hidden / 32)


@pytest.mark.parametrize("case", TIGHT, ids=TID)
def test_every_slot_real_and_a_tile_count_off_the_remap_unit(gpu, case):
    pkg = gpu
    counts, out, hidden = case
    inf = 192
    k = TIGHT.index(case)
    (fw, fx), o = PAIRS[k % 4], OUTS[k % 3]
    rng = np.random.default_rng(2150 + k)
    off, tokens, G = tight_layout(pkg, counts, out, inf, 0)
    pr = Problem(pkg, rng, fw, fx, o, G, out, inf, tokens)
    Yb, Y = run_plain(pr, off, out)
    compare_groups(pr, Y, off, out, lambda g, lo, hi: ref_plain(pr, g, lo, hi, out))
    off, tokens, G = tight_layout(pkg, counts, 2 * hidden, inf, 0)
    pr = Problem(pkg, rng, fw, fx, o, G, 2 * hidden, inf, tokens)
    Yb, Y = run_glu(pr, off, hidden, "relu")
    compare_groups(pr, Y, off, hidden, lambda g, lo, hi: ref_glu(pr, g, lo, hi, hidden, act="relu"))


EPIS = ["col_bias", "row_bias", "residual_in_place", "hardswish_col"]


@pytest.mark.parametrize("epi", EPIS)
def test_every_epilogue_per_group(gpu, epi):
    """A COL bias is expert-major (groups * out values), a ROW bias and the residual are in Y's global rows."""
    pkg = gpu
    out, inf = 77, 128
    counts = [5, 0, 70, 64]
    off, tokens = layout(counts)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, out, inf) == "tile64"
    k = EPIS.index(epi)
    o = OUTS[k % 3]
    rng = np.random.default_rng(2200 + k)
    pr = Problem(pkg, rng, *PAIRS[k], o, G, out, inf, tokens)
    colb, rowb = f32dev(rng.uniform(-2, 2, G * out)), f32dev(rng.uniform(-2, 2, tokens))
    R = torch.from_numpy(rng.uniform(-2, 2, (tokens, out)).astype(np.float32)).to(ODT[o]).to(DEV)
    E = pkg.Epilogue
    alpha, beta, fill, epi_all = 1.0, 0.0, None, None
    if epi in ("col_bias", "hardswish_col"):
        act = "relu" if epi == "col_bias" else "hardswish"
        epi_all = E(bias=colb, bias_dim="col", act=act)
        mk = lambda g, lo, n: dict(epilogue=E(bias=colb[g * out:(g + 1) * out], bias_dim="col", act=act))
    elif epi == "row_bias":
        epi_all = E(bias=rowb, bias_dim="row")
        mk = lambda g, lo, n: dict(epilogue=E(bias=torch.cat([rowb[lo:], torch.zeros(n, device=DEV)])[:n].contiguous(), bias_dim="row"))
    else:
        alpha, beta, fill = 0.5, 0.75, R

        def mk(g, lo, n):
            Y0 = torch.zeros((n, out), dtype=ODT[o], device=DEV)
            Y0[:min(n, tokens - lo)] = R[lo:lo + n]
            return dict(Y0=Y0)
    Yb, Y = run_plain(pr, off, out, epi=epi_all, alpha=alpha, beta=beta, fill=fill)
    check_untouched(pr, Yb, out, ranges(off, tokens))
    compare_groups(pr, Y, off, out, lambda g, lo, hi: ref_plain(pr, g, lo, hi, out, alpha=alpha, beta=beta, **mk(g, lo, max(hi - lo, 17))))


# ------------------------------------------------------------------------------------------------ 2. integer operands
@pytest.mark.parametrize("o", OUTS)
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=CID)
def test_integer_operands_give_the_fp64_product_rounded_once(gpu, case, o):
    """W: two of every four kept, values in {-2, -1, 1, 2}; X integers in [-2, 2]; in = 64: |acc| <= 32 * 4 = 128 < 2^8, an integer every
    output type holds exactly; no scales.  Y is the fp64 product, per group with that group's expert.  Gated with act NONE: |g u| <=
    16384 is exact in fp32 and rounded ONCE to the output type."""
    pkg = gpu
    form, _, hidden, _ = case
    inf = 64
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    k = CASES.index(case)
    fw, fx = PAIRS[(k + OUTS.index(o)) % 4]
    rng = np.random.default_rng(2300 + k)
    Wn = np.where(mask24(rng, G * 2 * hidden, inf), rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(G * 2 * hidden, inf)), 0.0)
    Xn = rng.integers(-2, 3, size=(tokens, inf)).astype(np.float64)
    assert pkg.linear24_grouped_form(tokens, G, 2 * hidden, inf) == form
    pr = Problem(pkg, rng, fw, fx, o, G, 2 * hidden, inf, tokens, W=Wn, X=Xn)
    Yb, Y = run_plain(pr, off, 2 * hidden, scales=False)
    check_untouched(pr, Yb, 2 * hidden, ranges(off, tokens))
    Yg = run_glu(pr, off, hidden, "none", scales=False)[1]
    for g, (lo, hi) in enumerate(ranges(off, tokens)):
        if hi == lo:
            continue
        acc = Xn[lo:hi] @ Wn[g * 2 * hidden:(g + 1) * 2 * hidden].T
        assert np.abs(acc).max() < 2 ** 8
        want = torch.from_numpy(acc).to(ODT[o])
        assert np.array_equal(want.double().numpy(), acc)
        assert_bits(Y[lo:hi, :2 * hidden].cpu(), want, f"plain group {g}")
        assert_bits(Yg[lo:hi, :hidden].cpu(), torch.from_numpy(acc[:, :hidden] * acc[:, hidden:]).to(ODT[o]), f"gated group {g}")


# ------------------------------------------------------------------------------------------------ 3. offsets out of contract
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_offsets_out_of_contract_touch_nothing_else(gpu, gated):
    """off[groups] > tokens, a negative off[0] and one decreasing pair.  X and Y carry guard rows inside their allocations, so even an
    unclamped kernel would stay in allocated memory; the guards must be intact and every row outside the overlap exact."""
    pkg = gpu
    inf, tokens = 192, 200
    rows = 82 if gated else 77
    width = rows // 2 if gated else rows
    off = [-2, 30, 90, 60, 150, tokens + 3]       # group 2 is empty (90 > 60); group 3's [60, 150) overlaps group 1's [30, 90) in [60, 90)
    G = len(off) - 1
    assert GUARD >= 3
    pr = Problem(pkg, np.random.default_rng(2400), "e4m3", "e5m2", "bf16", G, rows, inf, tokens)
    before = pr.Xbuf.view(torch.uint8).clone()
    Yb, Y = run_glu(pr, off, width, "relu") if gated else run_plain(pr, off, width)
    owned = ranges(off, tokens)
    assert owned == [(0, 30), (30, 90), (90, 90), (60, 150), (150, 200)]
    check_untouched(pr, Yb, width, owned)
    assert torch.equal(pr.Xbuf.view(torch.uint8), before)
    ref = (lambda g, lo, hi: ref_glu(pr, g, lo, hi, width, act="relu")) if gated else (lambda g, lo, hi: ref_plain(pr, g, lo, hi, width))
    for g, lo, hi in ((0, 0, 30), (1, 30, 60), (3, 90, 150), (4, 150, 200)):       # everything but the overlap [60, 90)
        assert_bits(Y[lo:hi, :width], ref(g, lo, hi), f"group {g} [{lo}, {hi})")


# ------------------------------------------------------------------------------------------------ 4. NaN, graphs
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_nan_reaches_exactly_the_rows_it_feeds(gpu, gated):
    pkg = gpu
    inf, rows = 128, 96
    width = rows // 2 if gated else rows
    counts = [20, 70, 0, 33]
    off, tokens = layout(counts, head=0, tail=0)
    G = len(counts)
    rng = np.random.default_rng(2500)
    keep = mask24(rng, G * rows, inf)
    Wn = np.where(keep, rng.uniform(0.25, 2.0, keep.shape) * rng.choice(np.array([-1.0, 1.0]), size=keep.shape), 0.0)
    Xn = rng.uniform(0.25, 2.0, (tokens, inf))
    wrow, wcol = 1 * rows + 9, int(np.flatnonzero(keep[1 * rows + 9])[3])      # a kept value of expert 1, row 9 (a gate row when gated)
    Wn[wrow, wcol] = np.nan
    tok, xcol = 95, 17                                                         # a token of group 3
    Xn[tok, xcol] = np.nan
    pr = Problem(pkg, rng, "e4m3", "e4m3", "f32", G, rows, inf, tokens, W=Wn, X=Xn)
    Y = (run_glu(pr, off, width, "none") if gated else run_plain(pr, off, width))[1]
    got = torch.isnan(Y[:, :width]).cpu().numpy()
    want = np.zeros((tokens, rows), dtype=bool)
    for g, (lo, hi) in enumerate(ranges(off, tokens)):
        if lo <= tok < hi:
            want[tok] |= keep[g * rows:(g + 1) * rows][:, xcol]
        if g == 1:
            want[lo:hi, 9] = True
    if gated:
        want = want[:, :width] | want[:, width:]
    assert want[tok].any() and not want[tok].all() and want[20:90, 9].all()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_hipgraph_replays_follow_the_offsets(gpu, gated):
    """Captured once; the routing then changes in device memory only.  Each replay equals its eager run bit for bit."""
    pkg = gpu
    inf, tokens, G = 192, 300, 4
    rows = 130 if gated else 77
    width = rows // 2 if gated else rows
    pr = Problem(pkg, np.random.default_rng(2600), "e4m3", "e4m3", "bf16", G, rows, inf, tokens)
    ldy = width + 4
    call = ((lambda Y, off: pkg.linear24_grouped_glu_fp8(pr.blob, pr.X, Y, off, G, tokens, width, inf, ldy=ldy, w_scale=pr.ws, x_scale=pr.xs, **pr.kw))
            if gated else
            (lambda Y, off: pkg.linear24_grouped_fp8(pr.blob, pr.X, Y, off, G, tokens, width, inf, ldy=ldy, w_scale=pr.ws, x_scale=pr.xs, **pr.kw)))
    routings = [[0, 100, 100, 230, 300], [10, 11, 140, 141, 290]]
    eager = []
    for r in routings:
        Ye = torch.full((tokens, ldy), SENTINEL, dtype=torch.bfloat16, device=DEV)
        call(Ye, i32dev(r))
        torch.cuda.synchronize()
        eager.append(Ye)
    assert not torch.equal(bits(eager[0]), bits(eager[1]))
    off = i32dev(routings[0])
    Y = torch.full((tokens, ldy), SENTINEL, dtype=torch.bfloat16, device=DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # one stream, one kernel node: no parallel branches
        call(Y, off)
    for r, Ye in list(zip(routings, eager)) + [(routings[0], eager[0])]:
        off.copy_(i32dev(r))
        Y.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(Y), bits(Ye)), f"replay under offsets {r} differs from the eager run"
