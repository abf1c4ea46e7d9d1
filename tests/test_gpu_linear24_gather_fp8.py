"""sm_linear24_grouped_gather_fp8 and sm_linear24_grouped_glu_gather_fp8 on the device: the grouped fp8 layers with X -- and x_scale, which
belongs to the token that was quantised -- read through a row index.

1. bit equality with sm_linear24_grouped_fp8 / sm_linear24_grouped_glu_fp8 on the materialised X.index_select(0, x_index) and
   x_scale.index_select(0, x_index), over the WHOLE guarded Y buffer, in every tile instantiation, plain and gated, on the shape list of
   test_gpu_linear24_grouped_fp8.py, for a permutation, the identity, a repeating index (x_rows < tokens) and x_rows > tokens; every
   format pair and output type on one shape.  The scales are distinct per row of X, and a per-token bias distinct per row of Y: reading
   either at the other's row changes bits;
2. indices out of contract read row 0 / row x_rows - 1 of X and of x_scale, never the NaN guard rows of X or the NaN guards of x_scale;
3. a NaN row of X reaches exactly the Y rows that index it;
4. a hipGraph replayed under a changed x_index and changed offsets equals the eager runs.
Every call runs on X with ldx > in, NaN bytes in the padding and NaN guard rows around the x_rows rows inside the same allocation, and on
a sentinel-filled Y with ldy > out and guard rows of its own.  Every case asks the form query -- with the device's compute units, as the
fp8 layers do -- which form it runs."""
import numpy as np
import pytest
import torch
from linear24_testlib import (BN, CID, DEV, GUARD, NAN_BYTE, ODT, OUTS, PAIRS, SENTINEL, TDT, dev8, encode8, f32dev, indices, layout, mask24,
                              ranges, sizes)

pytestmark = pytest.mark.gpu

IDT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


# form, out of the plain case (odd: per-element stores; % 4 == 0: packed), hidden of the gated one, in.  The sizes() of a 64-token tile are
# 401 tokens in 7 tiles, mean 51; those of a 128-token tile 785 tokens in 7 tiles, mean 99: 37 tile rows (> 4608 blob rows) reach 256 workgroups
CASES = [("tile64", 77, 41, 64), ("tile64", 84, 44, 192), ("tile128x64", 4613, 2307, 64), ("tile128x64", 4612, 2308, 320),
         ("tile128", 4613, 2307, 128), ("tile128", 4612, 2308, 192)]


def bits(t):
    return t.contiguous().view(IDT[t.dtype])


def i32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def compress(pkg, W8):
    rows, inf = W8.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 1, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24_fp8(W8.contiguous(), rows, inf, inf, 1, rows * inf, blob)
    return blob


class Problem:
    """groups experts W[g][rows][in] (2:4) as one stacked fp8 blob with w_scale (groups * rows, expert-major); `tokens` sorted rows of Y"""

    def __init__(self, pkg, rng, fw, fx, o, groups, rows, inf, tokens, W=None):
        self.pkg, self.fw, self.fx, self.o, self.groups, self.rows, self.inf, self.tokens = pkg, fw, fx, o, groups, rows, inf, tokens
        Wn = np.where(mask24(rng, groups * rows, inf), rng.uniform(-2, 2, (groups * rows, inf)), 0.0) if W is None else W
        self.blob = compress(pkg, dev8(encode8(Wn, fw), fw))
        self.ldx = inf + 16
        self.ws = f32dev(rng.uniform(0.5, 2.0, groups * rows))
        self.kw = dict(w_dtype=TDT[fw], ldx=self.ldx)

    def xbuf(self, Xn, rng):
        """x_rows rows as fp8 bytes in a NaN-padded buffer with NaN guard rows; x_scale, distinct per row, between NaN guards"""
        n = Xn.shape[0]
        xb = np.full((n + 2 * GUARD, self.ldx), NAN_BYTE[self.fx], dtype=np.uint8)
        xb[GUARD:GUARD + n, :self.inf] = encode8(Xn, self.fx)
        Xb = dev8(xb, self.fx)
        sb = np.full(n + 2 * GUARD, np.nan, dtype=np.float32)
        sb[GUARD:GUARD + n] = rng.permutation(n) / n + 0.5              # n distinct values in [0.5, 1.5)
        Sb = f32dev(sb)
        return Xb, Xb[GUARD:GUARD + n], Sb[GUARD:GUARD + n]

    def materialised(self, X, xs, idx):
        """X.index_select(0, x_index) and x_scale.index_select(0, x_index): what the parent's route hands the grouped layer"""
        sel = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(DEV)
        Xm = torch.full((self.tokens + 2 * GUARD, self.ldx), NAN_BYTE[self.fx], dtype=torch.uint8, device=DEV)
        Xm[GUARD:GUARD + self.tokens] = X.view(torch.uint8).index_select(0, sel)
        return Xm.view(TDT[self.fx])[GUARD:GUARD + self.tokens], xs.index_select(0, sel).contiguous()

    def run(self, X, xs, off, width, gated, x_index=None, x_rows=None, **kw):
        """the gathered layer (x_index given) or its grouped twin; returns the whole guarded Y buffer"""
        ldy = width + 12
        Yb = torch.full((self.tokens + 2 * GUARD, ldy), SENTINEL, dtype=ODT[self.o], device=DEV)
        Y = Yb[GUARD:GUARD + self.tokens]
        g = dict(x_index=i32dev(x_index), x_rows=x_rows) if x_index is not None else {}
        fn = self.pkg.linear24_grouped_glu_fp8 if gated else self.pkg.linear24_grouped_fp8
        fn(self.blob, X, Y, i32dev(off), self.groups, self.tokens, width, self.inf, ldy=ldy, w_scale=self.ws, x_scale=xs, **g, **self.kw, **kw)
        torch.cuda.synchronize()
        return Yb


def assert_bits(got, ref, what):
    bad = torch.nonzero(bits(got) != bits(ref))
    assert bad.numel() == 0, f"{what}: first mismatch at (row, column) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


def epilogue_kw(pkg, rng, gated, G, rows, tokens):
    if gated:
        return dict(act="silu", bias=f32dev(rng.uniform(-1, 1, G * rows)))
    return dict(epilogue=pkg.Epilogue(bias=f32dev(rng.uniform(-2, 2, tokens)), bias_dim="row"))       # a per-token bias stays in Y's sorted rows


# ------------------------------------------------------------------------------------------------ 1. every tile instantiation
@pytest.mark.parametrize("case", CASES, ids=CID)
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_gathered_equals_grouped_on_the_materialised_x(gpu, gated, case):
    pkg = gpu
    form, out, hidden, inf = case
    i = CASES.index(case)
    (fw, fx), o = PAIRS[(i + gated) % 4], OUTS[(i + 2 * gated) % 3]
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    rows, width = (2 * hidden, hidden) if gated else (out, out)
    assert pkg.linear24_grouped_form(tokens, G, rows, inf) == form
    rng = np.random.default_rng(5000 + 2 * i + gated)
    pr = Problem(pkg, rng, fw, fx, o, G, rows, inf, tokens)
    kw = epilogue_kw(pkg, rng, gated, G, rows, tokens)
    for name, x_rows, idx in indices(rng, tokens):
        Xb, X, xs = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)), rng)
        got = pr.run(X, xs, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
        Xm, xsm = pr.materialised(X, xs, idx)
        ref = pr.run(Xm, xsm, off, width, gated, **kw)
        assert_bits(got, ref, f"{name}: the guarded Y buffer")
        owned = ranges(off, tokens)
        assert bool((got[:GUARD + owned[0][0]] == SENTINEL).all()) and bool((got[GUARD + owned[-1][1]:] == SENTINEL).all()), "rows no group owns were written"
        assert not bool(torch.isnan(got).any())
    again = pr.run(X, xs, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
    assert torch.equal(bits(got), bits(again)), "two runs on the same inputs differ"


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_every_format_pair_and_output_type(gpu, gated):
    """One shape, both scales, x_scale in X's rows: 4 format pairs x 3 output types, a repeating index."""
    pkg = gpu
    rows, inf = (82, 192) if gated else (77, 192)
    width = rows // 2 if gated else rows
    counts = [0, 66, 1, 64]
    off, tokens = layout(counts, head=1, tail=2)
    G = len(counts)
    x_rows = 50
    assert pkg.linear24_grouped_form(tokens, G, rows, inf) == "tile64"
    for k, ((fw, fx), o) in enumerate((p, o) for p in PAIRS for o in OUTS):
        rng = np.random.default_rng(5100 + k)
        pr = Problem(pkg, rng, fw, fx, o, G, rows, inf, tokens)
        idx = rng.permutation(tokens) % x_rows
        Xb, X, xs = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)), rng)
        kw = dict(act="relu") if gated else dict(alpha=0.75)
        got = pr.run(X, xs, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
        Xm, xsm = pr.materialised(X, xs, idx)
        assert_bits(got, pr.run(Xm, xsm, off, width, gated, **kw), f"{fw} x {fx} -> {o}")
        # the scale is the SOURCE row's: with x_scale read at Y's row instead, the reference itself changes
        wrong = pr.run(Xm, xs.repeat(-(-tokens // x_rows))[:tokens].contiguous(), off, width, gated, **kw)
        assert not torch.equal(bits(got), bits(wrong))


# ------------------------------------------------------------------------------------------------ 2. indices out of contract
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_indices_out_of_contract_read_no_row_outside_x(gpu, gated):
    """negative indices read row 0, indices >= x_rows read row x_rows - 1 -- of X and of x_scale; the NaN guard rows of X and the NaN
    guards of x_scale inside the same allocations are never read: no NaN anywhere in Y, every row exact against the clamped index."""
    pkg = gpu
    inf, x_rows = 128, 150
    rows, width = (82, 41) if gated else (77, 77)
    counts = [40, 0, 70, 64, 3]
    off, tokens = layout(counts, head=2, tail=1)
    G = len(counts)
    rng = np.random.default_rng(5200 + gated)
    pr = Problem(pkg, rng, "e4m3", "e5m2", "bf16", G, rows, inf, tokens)
    idx = rng.integers(0, x_rows, tokens)
    bad = rng.permutation(tokens)[:40]
    idx[bad] = np.concatenate([-np.arange(1, GUARD + 1), x_rows + np.arange(GUARD), [-2 ** 31, 2 ** 31 - 1, -x_rows, 2 * x_rows], rng.integers(-10 ** 6, 0, 14),
                               rng.integers(x_rows, 10 ** 6, 14)])
    Xb, X, xs = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)), rng)
    kw = dict(act="relu") if gated else {}
    got = pr.run(X, xs, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
    assert not bool(torch.isnan(got).any()), "a NaN guard row of X or a NaN guard of x_scale was read"
    Xm, xsm = pr.materialised(X, xs, np.clip(idx, 0, x_rows - 1))
    assert_bits(got, pr.run(Xm, xsm, off, width, gated, **kw), "out-of-contract indices against the clamped index")


# ------------------------------------------------------------------------------------------------ 3. NaN, 4. graphs
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_a_nan_row_of_x_reaches_exactly_the_rows_that_index_it(gpu, gated):
    pkg = gpu
    inf, x_rows = 128, 60
    rows, width = (96, 48) if gated else (96, 96)
    counts = [20, 70, 0, 33]
    off, tokens = layout(counts, head=2, tail=3)
    G = len(counts)
    rng = np.random.default_rng(5300)
    keep = mask24(rng, G * rows, inf)
    Wn = np.where(keep, rng.uniform(0.25, 2.0, keep.shape) * rng.choice(np.array([-1.0, 1.0]), size=keep.shape), 0.0)
    pr = Problem(pkg, rng, "e4m3", "e4m3", "f16", G, rows, inf, tokens, W=Wn)
    Xn = rng.uniform(0.25, 2.0, (x_rows, inf))
    Xn[17, :] = np.nan
    idx = rng.integers(0, x_rows, tokens)
    idx[idx == 17] = 18
    hit = np.array([0, 1, 2, 5, 30, 95, 100, 124, 127])           # unowned rows (0, 1 and the tail) and rows of groups 0, 1 and 3
    idx[hit] = 17
    Xb, X, xs = pr.xbuf(Xn, rng)
    got = pr.run(X, xs, off, width, gated, x_index=idx, x_rows=x_rows, **(dict(act="none") if gated else {}))
    Y = got[GUARD:GUARD + tokens, :width]
    want = np.zeros(tokens, dtype=bool)
    for lo, hi in ranges(off, tokens):
        want[lo:hi] = idx[lo:hi] == 17
    assert want.sum() == 6
    nan = torch.isnan(Y).cpu().numpy()
    assert np.array_equal(nan.all(axis=1), want) and np.array_equal(nan.any(axis=1), want)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_hipgraph_replays_follow_the_index_and_the_offsets(gpu, gated):
    """Captured once; x_index and the offsets then change in device memory only.  Each replay equals its eager run bit for bit."""
    pkg = gpu
    inf, tokens, G, x_rows = 192, 300, 4, 170
    rows, width = (130, 65) if gated else (77, 77)
    rng = np.random.default_rng(5400)
    pr = Problem(pkg, rng, "e5m2", "e4m3", "bf16", G, rows, inf, tokens)
    Xb, X, xs = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)), rng)
    ldy = width + 4
    fn = pkg.linear24_grouped_glu_fp8 if gated else pkg.linear24_grouped_fp8
    call = lambda Y, off, idx: fn(pr.blob, X, Y, off, G, tokens, width, inf, ldy=ldy, w_scale=pr.ws, x_scale=xs, x_index=idx, x_rows=x_rows, **pr.kw)
    routings = [([0, 100, 100, 230, 300], rng.integers(0, x_rows, tokens)), ([10, 11, 140, 141, 290], rng.integers(0, x_rows, tokens))]
    eager = []
    for off, idx in routings:
        Ye = torch.full((tokens, ldy), SENTINEL, dtype=torch.bfloat16, device=DEV)
        call(Ye, i32dev(off), i32dev(idx))
        torch.cuda.synchronize()
        eager.append(Ye)
    assert not torch.equal(bits(eager[0]), bits(eager[1]))
    d_off, d_idx = i32dev(routings[0][0]), i32dev(routings[0][1])
    Y = torch.full((tokens, ldy), SENTINEL, dtype=torch.bfloat16, device=DEV)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # one stream, one kernel node: no parallel branches
        call(Y, d_off, d_idx)
    for (off, idx), Ye in list(zip(routings, eager)) + [(routings[0], eager[0])]:
        d_off.copy_(i32dev(off))
        d_idx.copy_(i32dev(idx))
        Y.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(Y), bits(Ye)), f"replay under offsets {off} differs from the eager run"
