"""sm_linear24_grouped_{f16,bf16} and sm_linear24_grouped_glu_{f16,bf16} on the device: `groups` experts of one shape, tokens sorted
by expert, the per-expert offsets read from device memory, one launch.

1. bit equality per group with the plain layer (sm_linear24_* / sm_linear24_glu_*) on that slice of X and expert g's blob compressed
   alone, in every tile instantiation, plain and gated: group sizes 0 (first, middle, last), 1, BN - 1, BN, BN + 1 and several tiles,
   off[0] > 0 and off[groups] < tokens, odd and packed widths, in = 64 (shorter than the ring), every epilogue, every GLU act;
2. integer operands: the fp64 product rounded once, per group;
3. offsets out of contract: nothing outside the `tokens` rows is touched, every row outside the overlap is exact;
4. NaN reaches exactly the rows it feeds; two runs and hipGraph replays under changed offsets give the eager bits;
5. spmma_plan_t::linear_grouped / linear_glu_grouped against the C ABI (examples/bin/linear24_grouped).
Every call runs on X with ldx > in, NaN in the padding and NaN guard rows before and behind the tokens inside the same allocation, and
on a sentinel-filled Y with ldy > out and guard rows of its own.  Every case asks the form queries which form it runs -- at the 256
compute units the 16-bit layers ask the rule with."""
import os
import subprocess

import numpy as np
import pytest
import torch
from linear24_testlib import BN, CID, CUS, DEV, DT, GUARD, SENTINEL, TID, TIGHT, TYPES, f32dev, layout, mask24, ranges, sizes, tight_layout, todev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# form, out of the plain case (odd: per-element stores; % 4 == 0: packed), hidden of the gated one, in.  The sizes() of a 64-token tile are
# 401 tokens in 7 tiles, mean 51; those of a 128-token tile 785 tokens in 7 tiles, mean 99: 37 tile rows (> 4608 blob rows) reach 256 workgroups
CASES = [("tile64", 77, 41, 64), ("tile64", 84, 44, 192), ("tile128x64", 4613, 2307, 64), ("tile128x64", 4612, 2308, 320),
         ("tile128", 4613, 2307, 64), ("tile128", 4612, 2308, 192)]


def bits(t):
    return t.contiguous().view(torch.int16)


def i32dev(a):
    return torch.tensor([int(v) for v in a], dtype=torch.int32, device=DEV)


def compress(pkg, W):
    rows, inf = W.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 2, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24(W.contiguous(), rows, inf, inf, 1, rows * inf, blob)
    return blob


class Problem:
    """groups experts W[g][rows][in] (2:4, U(-2, 2)), X[tokens][in] in guarded, padded buffers; the stacked blob and each expert's own"""

    def __init__(self, pkg, rng, ty, groups, rows, inf, tokens, W=None, X=None):
        self.pkg, self.ty, self.groups, self.rows, self.inf, self.tokens = pkg, ty, groups, rows, inf, tokens
        Wn = np.where(mask24(rng, groups * rows, inf), rng.uniform(-2, 2, (groups * rows, inf)), 0.0) if W is None else W
        Xn = rng.uniform(-2, 2, (tokens, inf)) if X is None else X
        self.W = todev(Wn, ty)
        self.blob = compress(pkg, self.W)
        self.own = [compress(pkg, self.W[g * rows:(g + 1) * rows]) for g in range(groups)]
        self.ldx = inf + 16
        self.Xbuf = torch.full((tokens + 2 * GUARD, self.ldx), float("nan"), dtype=DT[ty], device=DEV)
        self.X = self.Xbuf[GUARD:GUARD + tokens]
        self.X[:, :inf] = todev(Xn, ty)

    def ybuf(self, width, fill=None):
        ldy = width + 12
        Yb = torch.full((self.tokens + 2 * GUARD, ldy), SENTINEL, dtype=DT[self.ty], device=DEV)
        if fill is not None:
            Yb[GUARD:GUARD + self.tokens, :width] = fill
        self.before = Yb.clone()
        return Yb, ldy

    def slice_x(self, lo, hi):
        """rows lo .. hi-1 of X padded with zero rows to >= 17 tokens: the plain call then runs a tile form"""
        n = max(hi - lo, 17)
        Xs = torch.zeros((n, self.ldx), dtype=DT[self.ty], device=DEV)
        Xs[:hi - lo] = self.X[lo:hi]
        Xs[:, self.inf:] = float("nan")
        return Xs, n


def check_untouched(pr, Yb, width, tokens, owned):
    """guard rows, slack columns and rows no group owns keep the bits they had (the sentinel's; a residual's where Y was one)"""
    free = torch.ones(tokens + 2 * GUARD, dtype=torch.bool, device=DEV)
    for lo, hi in owned:
        free[GUARD + lo:GUARD + hi] = False
    assert torch.equal(bits(Yb[free]), bits(pr.before[free])), "a row no group owns, or a guard row, was written"
    assert bool((Yb[:, width:] == SENTINEL).all()), "columns at or beyond the width of Y were written"


def assert_bits(got, ref, what):
    bad = torch.nonzero(bits(got) != bits(ref))
    assert bad.numel() == 0, f"{what}: first mismatch at (token, feature) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


def run_plain(pr, off, out, epi=None, alpha=1.0, beta=0.0, fill=None):
    pkg = pr.pkg
    Yb, ldy = pr.ybuf(out, fill)
    Y = Yb[GUARD:GUARD + pr.tokens]
    pkg.linear24_grouped(pr.blob, pr.X, Y, i32dev(off), pr.groups, pr.tokens, out, pr.inf, ldx=pr.ldx, ldy=ldy, alpha=alpha, beta=beta, epilogue=epi)
    torch.cuda.synchronize()
    return Yb, Y


def run_glu(pr, off, hidden, act="silu", bias=None):
    pkg = pr.pkg
    Yb, ldy = pr.ybuf(hidden)
    Y = Yb[GUARD:GUARD + pr.tokens]
    pkg.linear24_grouped_glu(pr.blob, pr.X, Y, i32dev(off), pr.groups, pr.tokens, hidden, pr.inf, act=act, bias=bias, ldx=pr.ldx, ldy=ldy)
    torch.cuda.synchronize()
    return Yb, Y


def ref_plain(pr, g, lo, hi, out, **kw):
    Xs, n = pr.slice_x(lo, hi)
    assert pr.pkg.linear24_fp8_form(n, out, pr.inf, cus=CUS).startswith("tile")
    Yr = torch.full((n, out), SENTINEL, dtype=DT[pr.ty], device=DEV) if "Y0" not in kw else kw.pop("Y0")
    pr.pkg.linear24(pr.own[g], Xs, Yr, n, out, pr.inf, ldx=pr.ldx, **kw)
    torch.cuda.synchronize()
    return Yr[:hi - lo]


def ref_glu(pr, g, lo, hi, hidden, **kw):
    Xs, n = pr.slice_x(lo, hi)
    assert pr.pkg.linear24_glu_form(n, hidden, pr.inf, cus=CUS).startswith("tile")
    Yr = torch.full((n, hidden), SENTINEL, dtype=DT[pr.ty], device=DEV)
    pr.pkg.linear24_glu(pr.own[g], Xs, Yr, n, hidden, pr.inf, ldx=pr.ldx, **kw)
    torch.cuda.synchronize()
    return Yr[:hi - lo]


# ------------------------------------------------------------------------------------------------ 1. every tile instantiation
@pytest.mark.parametrize("case", CASES, ids=CID)
@pytest.mark.parametrize("ty", TYPES)
def test_plain_groups_equal_the_plain_layer_bit_for_bit(gpu, ty, case):
    pkg = gpu
    form, out, _, inf = case
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, out, inf, cus=CUS) == form
    pr = Problem(pkg, np.random.default_rng(1000 + CASES.index(case)), ty, G, out, inf, tokens)
    Yb, Y = run_plain(pr, off, out)
    owned = ranges(off, tokens)
    check_untouched(pr, Yb, out, tokens, owned)
    for g, (lo, hi) in enumerate(owned):
        if hi > lo:
            assert_bits(Y[lo:hi, :out], ref_plain(pr, g, lo, hi, out), f"group {g} [{lo}, {hi})")
    again, _ = run_plain(pr, off, out)
    assert torch.equal(bits(Yb), bits(again)), "two runs on the same inputs differ"


@pytest.mark.parametrize("case", CASES, ids=CID)
@pytest.mark.parametrize("ty", TYPES)
def test_gated_groups_equal_the_gated_layer_bit_for_bit(gpu, ty, case):
    pkg = gpu
    form, _, hidden, inf = case
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, 2 * hidden, inf, cus=CUS) == form
    rng = np.random.default_rng(1100 + CASES.index(case))
    pr = Problem(pkg, rng, ty, G, 2 * hidden, inf, tokens)
    bias = f32dev(rng.uniform(-1, 1, G * 2 * hidden))
    Yb, Y = run_glu(pr, off, hidden, "silu", bias)
    owned = ranges(off, tokens)
    check_untouched(pr, Yb, hidden, tokens, owned)
    for g, (lo, hi) in enumerate(owned):
        if hi > lo:
            ref = ref_glu(pr, g, lo, hi, hidden, act="silu", bias=bias[g * 2 * hidden:(g + 1) * 2 * hidden])
            assert_bits(Y[lo:hi, :hidden], ref, f"group {g} [{lo}, {hi})")
    again, _ = run_glu(pr, off, hidden, "silu", bias)
    assert torch.equal(bits(Yb), bits(again)), "two runs on the same inputs differ"


# ------------------------------------------------------------------------------------------------ 1b. every slot real, T % 8 != 0
# Routings that ATTAIN the slot bound min(tokens, ceil(tokens / 64) + groups - 1) -- no block of the grid is spare -- with a real-tile
# count T = tiles_m * slots that is no multiple of 8 (the XCD remap's unit): one group; one token per group; counts = 1 mod 64.
# (counts, out of the plain case, hidden of the gated one): tiles_m = ceil(out / 64) = ceil(hidden / 32)


@pytest.mark.parametrize("case", TIGHT, ids=TID)
@pytest.mark.parametrize("ty", TYPES)
def test_every_slot_real_and_a_tile_count_off_the_remap_unit(gpu, ty, case):
    pkg = gpu
    counts, out, hidden = case
    inf = 128
    rng = np.random.default_rng(1150 + TIGHT.index(case))
    off, tokens, G = tight_layout(pkg, counts, out, inf, CUS)
    pr = Problem(pkg, rng, ty, G, out, inf, tokens)
    Yb, Y = run_plain(pr, off, out)
    for g, (lo, hi) in enumerate(ranges(off, tokens)):
        assert_bits(Y[lo:hi, :out], ref_plain(pr, g, lo, hi, out), f"plain group {g} [{lo}, {hi})")
    off, tokens, G = tight_layout(pkg, counts, 2 * hidden, inf, CUS)
    pr = Problem(pkg, rng, ty, G, 2 * hidden, inf, tokens)
    Yb, Y = run_glu(pr, off, hidden, "relu")
    for g, (lo, hi) in enumerate(ranges(off, tokens)):
        assert_bits(Y[lo:hi, :hidden], ref_glu(pr, g, lo, hi, hidden, act="relu"), f"gated group {g} [{lo}, {hi})")


EPIS = ["col_bias", "row_bias", "residual_in_place", "residual_and_leaky", "hardswish_col"]


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("ty", TYPES)
def test_every_epilogue_per_group(gpu, ty, epi):
    """A COL bias is expert-major (groups * out values), a ROW bias and the residual are in Y's global rows."""
    pkg = gpu
    out, inf = 77, 128
    counts = [5, 0, 70, 64]
    off, tokens = layout(counts)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, out, inf, cus=CUS) == "tile64"
    rng = np.random.default_rng(1200 + EPIS.index(epi))
    pr = Problem(pkg, rng, ty, G, out, inf, tokens)
    colb, rowb = f32dev(rng.uniform(-2, 2, G * out)), f32dev(rng.uniform(-2, 2, tokens))
    R = todev(rng.uniform(-2, 2, (tokens, out)), ty)
    E = pkg.Epilogue
    alpha, beta, fill = 1.0, 0.0, None
    if epi == "col_bias":
        mk = lambda g, lo, n: E(bias=colb[g * out:(g + 1) * out], bias_dim="col", act="relu")
        epi_all = E(bias=colb, bias_dim="col", act="relu")
    elif epi == "row_bias":
        pad = lambda lo, n: torch.cat([rowb[lo:], torch.zeros(n, device=DEV)])[:n].contiguous()
        mk = lambda g, lo, n: E(bias=pad(lo, n), bias_dim="row")
        epi_all = E(bias=rowb, bias_dim="row")
    elif epi == "residual_in_place":
        alpha, beta, fill = 0.5, 0.75, R
        mk = lambda g, lo, n: None
        epi_all = None
    elif epi == "residual_and_leaky":
        alpha, beta = 1.5, -0.5
        mk = None
        epi_all = None
    else:
        mk = lambda g, lo, n: E(bias=colb[g * out:(g + 1) * out], bias_dim="col", act="hardswish")
        epi_all = E(bias=colb, bias_dim="col", act="hardswish")
    if epi == "residual_and_leaky":
        Rb, ldy = pr.ybuf(out, R)                    # a residual of Y's shape and ldy, not Y
        epi_all = E(act="leaky_relu", act_arg=0.1, residual=Rb[GUARD:GUARD + tokens])
    Yb, Y = run_plain(pr, off, out, epi=epi_all, alpha=alpha, beta=beta, fill=fill)
    owned = ranges(off, tokens)
    check_untouched(pr, Yb, out, tokens, owned)
    for g, (lo, hi) in enumerate(owned):
        if hi == lo:
            continue
        n = max(hi - lo, 17)
        if epi in ("residual_in_place", "residual_and_leaky"):
            Y0 = torch.zeros((n, out), dtype=DT[ty], device=DEV)
            Y0[:hi - lo] = R[lo:hi]
            if epi == "residual_in_place":
                ref = ref_plain(pr, g, lo, hi, out, alpha=alpha, beta=beta, Y0=Y0)
            else:
                ref = ref_plain(pr, g, lo, hi, out, alpha=alpha, beta=beta, epilogue=E(act="leaky_relu", act_arg=0.1, residual=Y0))
        else:
            ref = ref_plain(pr, g, lo, hi, out, epilogue=mk(g, lo, n))
        assert_bits(Y[lo:hi, :out], ref, f"{epi} group {g}")


@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_every_glu_act_per_group(gpu, act):
    pkg = gpu
    hidden, inf, ty = 41, 64, "f16"
    counts = [0, 66, 1, 64]
    off, tokens = layout(counts, head=1, tail=0)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, 2 * hidden, inf, cus=CUS) == "tile64"
    pr = Problem(pkg, np.random.default_rng(1300), ty, G, 2 * hidden, inf, tokens)
    Yb, Y = run_glu(pr, off, hidden, act)
    owned = ranges(off, tokens)
    check_untouched(pr, Yb, hidden, tokens, owned)
    for g, (lo, hi) in enumerate(owned):
        if hi > lo:
            assert_bits(Y[lo:hi, :hidden], ref_glu(pr, g, lo, hi, hidden, act=act), f"{act} group {g}")


# ------------------------------------------------------------------------------------------------ 2. integer operands
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=CID)
def test_integer_operands_give_the_fp64_product_rounded_once(gpu, case, ty):
    """W in {-1, 0, 1} (two kept of four), X integers in [-3, 3], in = 64: |acc| <= 32 * 3 = 96 < 2^8, an integer both 16-bit types hold
    exactly -- Y is the fp64 product, per group with that group's expert.  Gated with act NONE: |g u| <= 9216, exact in fp32, rounded
    ONCE to the output type."""
    pkg = gpu
    form, _, hidden, inf = case
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    rng = np.random.default_rng(1400 + CASES.index(case))
    Wn = np.where(mask24(rng, G * 2 * hidden, inf), rng.choice(np.array([-1.0, 1.0]), size=(G * 2 * hidden, inf)), 0.0)
    Xn = rng.integers(-3, 4, size=(tokens, inf)).astype(np.float64)
    pr = Problem(pkg, rng, ty, G, 2 * hidden, inf, tokens, W=Wn, X=Xn)
    assert pkg.linear24_grouped_form(tokens, G, 2 * hidden, inf, cus=CUS) == form
    Yb, Y = run_plain(pr, off, 2 * hidden)
    check_untouched(pr, Yb, 2 * hidden, tokens, ranges(off, tokens))
    Yg = run_glu(pr, off, hidden, "none")[1]
    for g, (lo, hi) in enumerate(ranges(off, tokens)):
        if hi == lo:
            continue
        acc = Xn[lo:hi] @ Wn[g * 2 * hidden:(g + 1) * 2 * hidden].T
        assert np.abs(acc).max() < 2 ** 8
        want = torch.from_numpy(acc).to(DT[ty])
        assert np.array_equal(want.double().numpy(), acc)
        assert_bits(Y[lo:hi, :2 * hidden].cpu(), want, f"plain group {g}")
        assert_bits(Yg[lo:hi, :hidden].cpu(), torch.from_numpy(acc[:, :hidden] * acc[:, hidden:]).to(DT[ty]), f"gated group {g}")


# ------------------------------------------------------------------------------------------------ 3. offsets out of contract
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_offsets_out_of_contract_touch_nothing_else(gpu, gated):
    """off[groups] > tokens, a negative off[0] and one decreasing pair.  X and Y carry guard rows inside their allocations, so even an
    unclamped kernel would stay in allocated memory; the guards must be intact and every row outside the overlap exact."""
    pkg = gpu
    ty, inf, tokens = "bf16", 128, 200
    rows = 82 if gated else 77
    width = rows // 2 if gated else rows
    off = [-2, 30, 90, 60, 150, tokens + 3]       # group 2 is empty (90 > 60); group 3's [60, 150) overlaps group 1's [30, 90) in [60, 90)
    G = len(off) - 1
    assert GUARD >= 3
    pr = Problem(pkg, np.random.default_rng(1500), ty, G, rows, inf, tokens)
    Yb, Y = run_glu(pr, off, width, "relu") if gated else run_plain(pr, off, width)
    owned = ranges(off, tokens)
    assert owned == [(0, 30), (30, 90), (90, 90), (60, 150), (150, 200)]
    check_untouched(pr, Yb, width, tokens, owned)
    assert bool(torch.isnan(pr.Xbuf[:GUARD]).all()) and bool(torch.isnan(pr.Xbuf[GUARD + tokens:]).all())
    ref = (lambda g, lo, hi: ref_glu(pr, g, lo, hi, width, act="relu")) if gated else (lambda g, lo, hi: ref_plain(pr, g, lo, hi, width))
    for g, lo, hi in ((0, 0, 30), (1, 30, 60), (3, 90, 150), (4, 150, 200)):       # everything but the overlap [60, 90)
        assert_bits(Y[lo:hi, :width], ref(g, lo, hi), f"group {g} [{lo}, {hi})")


# ------------------------------------------------------------------------------------------------ 4. NaN, graphs
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_nan_reaches_exactly_the_rows_it_feeds(gpu, gated):
    pkg = gpu
    ty, inf = "f16", 128
    rows = 96
    width = rows // 2 if gated else rows
    counts = [20, 70, 0, 33]
    off, tokens = layout(counts, head=0, tail=0)
    G = len(counts)
    rng = np.random.default_rng(1600)
    keep = mask24(rng, G * rows, inf)
    sign = rng.choice(np.array([-1.0, 1.0]), size=keep.shape)
    Wn = np.where(keep, rng.uniform(0.25, 2.0, keep.shape) * sign, 0.0)
    Xn = rng.uniform(0.25, 2.0, (tokens, inf))
    wrow, wcol = 1 * rows + 9, int(np.flatnonzero(keep[1 * rows + 9])[3])      # a kept value of expert 1, row 9 (a gate row when gated)
    Wn[wrow, wcol] = np.nan
    tok, xcol = 95, 17                                                         # a token of group 3
    Xn[tok, xcol] = np.nan
    pr = Problem(pkg, rng, ty, G, rows, inf, tokens, W=Wn, X=Xn)
    Y = (run_glu(pr, off, width, "none") if gated else run_plain(pr, off, width))[1]
    got = torch.isnan(Y[:, :width]).cpu().numpy()
    want = np.zeros((tokens, rows), dtype=bool)
    for g, (lo, hi) in enumerate(ranges(off, tokens)):
        kg = keep[g * rows:(g + 1) * rows]
        if lo <= tok < hi:
            want[tok] |= kg[:, xcol]
        if g == 1:
            want[lo:hi, 9] = True
    if gated:
        want = want[:, :width] | want[:, width:]
    assert want[tok].any() and not want[tok].all() and want[20:90, 9].all()
    assert np.array_equal(got, want)
    assert bool(torch.isfinite(Y[:20, :width].float()).all())                  # expert 0's rows: untouched by expert 1's NaN


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_hipgraph_replays_follow_the_offsets(gpu, gated):
    """Captured once; the routing then changes in device memory only.  Each replay equals its eager run bit for bit."""
    pkg = gpu
    ty, inf, tokens, G = "bf16", 192, 300, 4
    rows = 130 if gated else 77
    width = rows // 2 if gated else rows
    pr = Problem(pkg, np.random.default_rng(1700), ty, G, rows, inf, tokens)
    ldy = width + 4
    call = ((lambda Y, off: pkg.linear24_grouped_glu(pr.blob, pr.X, Y, off, G, tokens, width, inf, ldx=pr.ldx, ldy=ldy)) if gated else
            (lambda Y, off: pkg.linear24_grouped(pr.blob, pr.X, Y, off, G, tokens, width, inf, ldx=pr.ldx, ldy=ldy)))
    routings = [[0, 100, 100, 230, 300], [10, 11, 140, 141, 290]]
    eager = []
    for r in routings:
        Ye = torch.full((tokens, ldy), SENTINEL, dtype=DT[ty], device=DEV)
        call(Ye, i32dev(r))
        torch.cuda.synchronize()
        eager.append(Ye)
    assert not torch.equal(bits(eager[0]), bits(eager[1]))
    off = i32dev(routings[0])
    Y = torch.full((tokens, ldy), SENTINEL, dtype=DT[ty], device=DEV)
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


# ------------------------------------------------------------------------------------------------ 5. the C++ header mirror
def test_cpp_header_mirror(gpu):
    """examples/bin/linear24_grouped: spmma_plan_t::linear_glu_grouped then linear_grouped on a seeded random routing, against the C ABI
    and against the per-expert plan calls; the example checks itself and exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "linear24_grouped")
    assert os.path.exists(exe), "examples/bin/linear24_grouped is missing: build() makes it"
    res = subprocess.run([exe, "4", "128", "192", "300"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "equal to the C ABI bit for bit: yes" in res.stdout and "equal to the per-expert calls bit for bit: yes" in res.stdout
