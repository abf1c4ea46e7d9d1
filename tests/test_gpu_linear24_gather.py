"""sm_linear24_grouped_gather_{f16,bf16} and sm_linear24_grouped_glu_gather_{f16,bf16} on the device: the grouped layers with X read through
a row index (row t of Y reads row clamp(x_index[t], 0, x_rows - 1) of X).

1. bit equality with sm_linear24_grouped_* / sm_linear24_grouped_glu_* on the materialised X.index_select(0, x_index), over the WHOLE
   guarded Y buffer (so rows no group owns stay unwritten here as there), in every tile instantiation, plain and gated, on the shape
   list of test_gpu_linear24_grouped.py, for: a permutation; the identity; an index that repeats every source row (x_rows < tokens: the
   top_k copies of a token land in different groups); x_rows > tokens;
2. indices out of contract (negative, >= x_rows): they read row 0 / row x_rows - 1, never the NaN guard rows around X;
3. a NaN row of X reaches exactly the Y rows that index it;
4. a hipGraph replayed under a changed x_index and changed offsets equals the eager runs;
5. spmma_plan_t's x_index overloads against the C ABI (examples/bin/moe_block).
Every call runs on X with ldx > in, NaN in the padding and NaN guard rows before and behind the x_rows rows inside the same allocation,
and on a sentinel-filled Y with ldy > out and guard rows of its own.  Every case asks the form query which form it runs -- at the 256
compute units the 16-bit layers ask the rule with."""
import os
import subprocess

import numpy as np
import pytest
import torch
from linear24_testlib import BN, CID, CUS, DEV, DT, GUARD, SENTINEL, TYPES, f32dev, indices, layout, mask24, ranges, sizes, todev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# form, out of the plain case (odd: per-element stores; % 4 == 0: packed), hidden of the gated one, in.  The sizes() of a 64-token tile are
# 401 tokens in 7 tiles, mean 51; those of a 128-token tile 785 tokens in 7 tiles, mean 99: 37 tile rows (> 4608 blob rows) reach 256 workgroups
CASES = [("tile64", 77, 41, 64), ("tile64", 84, 44, 192), ("tile128x64", 4613, 2307, 64), ("tile128x64", 4612, 2308, 320),
         ("tile128", 4613, 2307, 64), ("tile128", 4612, 2308, 192)]


def bits(t):
    return t.contiguous().view(torch.int16)


def i32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def compress(pkg, W):
    rows, inf = W.shape
    blob = torch.empty(pkg.compress24_size(rows, inf, 2, 1), dtype=torch.uint8, device=DEV)
    pkg.compress24(W.contiguous(), rows, inf, inf, 1, rows * inf, blob)
    return blob


class Problem:
    """groups experts W[g][rows][in] (2:4, U(-2, 2)) as one stacked blob; `tokens` sorted rows of Y"""

    def __init__(self, pkg, rng, ty, groups, rows, inf, tokens, W=None):
        self.pkg, self.ty, self.groups, self.rows, self.inf, self.tokens = pkg, ty, groups, rows, inf, tokens
        Wn = np.where(mask24(rng, groups * rows, inf), rng.uniform(-2, 2, (groups * rows, inf)), 0.0) if W is None else W
        self.blob = compress(pkg, todev(Wn, ty))
        self.ldx = inf + 16

    def xbuf(self, Xn):
        """x_rows rows in a NaN-padded buffer with NaN guard rows around them; returns (buffer, the x_rows rows)"""
        n = Xn.shape[0]
        Xb = torch.full((n + 2 * GUARD, self.ldx), float("nan"), dtype=DT[self.ty], device=DEV)
        Xb[GUARD:GUARD + n, :self.inf] = todev(Xn, self.ty)
        return Xb, Xb[GUARD:GUARD + n]

    def materialised(self, X, idx):
        """X.index_select(0, x_index) in a guarded, padded buffer of its own: what the parent's route hands the grouped layer"""
        Xm = torch.full((self.tokens + 2 * GUARD, self.ldx), float("nan"), dtype=DT[self.ty], device=DEV)
        Xm[GUARD:GUARD + self.tokens] = X.index_select(0, torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(DEV))
        return Xm[GUARD:GUARD + self.tokens]

    def ybuf(self, width):
        ldy = width + 12
        return torch.full((self.tokens + 2 * GUARD, ldy), SENTINEL, dtype=DT[self.ty], device=DEV), ldy

    def run(self, X, off, width, gated, x_index=None, x_rows=None, **kw):
        """the gathered layer (x_index given) or its grouped twin; returns the whole guarded Y buffer"""
        Yb, ldy = self.ybuf(width)
        Y = Yb[GUARD:GUARD + self.tokens]
        g = dict(x_index=i32dev(x_index), x_rows=x_rows) if x_index is not None else {}
        if gated:
            self.pkg.linear24_grouped_glu(self.blob, X, Y, i32dev(off), self.groups, self.tokens, width, self.inf, ldx=self.ldx, ldy=ldy, **g, **kw)
        else:
            self.pkg.linear24_grouped(self.blob, X, Y, i32dev(off), self.groups, self.tokens, width, self.inf, ldx=self.ldx, ldy=ldy, **g, **kw)
        torch.cuda.synchronize()
        return Yb


def assert_bits(got, ref, what):
    bad = torch.nonzero(bits(got) != bits(ref))
    assert bad.numel() == 0, f"{what}: first mismatch at (row, column) {bad[0].tolist()}, {len(bad)} of {got.numel()}"


# ------------------------------------------------------------------------------------------------ 1. every tile instantiation
@pytest.mark.parametrize("case", CASES, ids=CID)
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("ty", TYPES)
def test_gathered_equals_grouped_on_the_materialised_x(gpu, ty, gated, case):
    pkg = gpu
    form, out, hidden, inf = case
    counts = sizes(BN[form])
    off, tokens = layout(counts)
    G = len(counts)
    rows, width = (2 * hidden, hidden) if gated else (out, out)
    assert pkg.linear24_grouped_form(tokens, G, rows, inf, cus=CUS) == form
    rng = np.random.default_rng(4000 + 2 * CASES.index(case) + gated)
    pr = Problem(pkg, rng, ty, G, rows, inf, tokens)
    kw = {}
    if gated:
        kw = dict(act="silu", bias=f32dev(rng.uniform(-1, 1, G * rows)))
    else:
        kw = dict(epilogue=pkg.Epilogue(bias=f32dev(rng.uniform(-2, 2, tokens)), bias_dim="row"))     # a per-token bias stays in Y's sorted rows
    for name, x_rows, idx in indices(rng, tokens):
        Xb, X = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)))
        got = pr.run(X, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
        ref = pr.run(pr.materialised(X, idx), off, width, gated, **kw)
        assert_bits(got, ref, f"{name}: the guarded Y buffer")
        owned = ranges(off, tokens)
        assert bool((got[:GUARD + owned[0][0]] == SENTINEL).all()) and bool((got[GUARD + owned[-1][1]:] == SENTINEL).all()), "rows no group owns were written"
        assert not bool(torch.isnan(got).any())
    again = pr.run(X, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
    assert torch.equal(bits(got), bits(again)), "two runs on the same inputs differ"


# ------------------------------------------------------------------------------------------------ 2. indices out of contract
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("ty", TYPES)
def test_indices_out_of_contract_read_no_row_outside_x(gpu, ty, gated):
    """negative indices read row 0, indices >= x_rows read row x_rows - 1; the NaN guard rows around X inside the same allocation (GUARD of
    them: an unclamped -1 .. -GUARD or x_rows .. x_rows + GUARD - 1 would land there) are never read: no NaN anywhere in Y, and every
    row, valid index or not, is exact against the clamped index."""
    pkg = gpu
    inf, x_rows = 128, 150
    rows, width = (82, 41) if gated else (77, 77)
    counts = [40, 0, 70, 64, 3]
    off, tokens = layout(counts, head=2, tail=1)
    G = len(counts)
    rng = np.random.default_rng(4100 + gated)
    pr = Problem(pkg, rng, ty, G, rows, inf, tokens)
    idx = rng.integers(0, x_rows, tokens)
    bad = rng.permutation(tokens)[:40]
    idx[bad] = np.concatenate([-np.arange(1, GUARD + 1), x_rows + np.arange(GUARD), [-2 ** 31, 2 ** 31 - 1, -x_rows, 2 * x_rows], rng.integers(-10 ** 6, 0, 14),
                               rng.integers(x_rows, 10 ** 6, 14)])
    Xb, X = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)))
    kw = dict(act="relu") if gated else {}
    got = pr.run(X, off, width, gated, x_index=idx, x_rows=x_rows, **kw)
    assert not bool(torch.isnan(got).any()), "a NaN guard row of X was read"
    ref = pr.run(pr.materialised(X, np.clip(idx, 0, x_rows - 1)), off, width, gated, **kw)
    assert_bits(got, ref, "out-of-contract indices against the clamped index")
    assert bool(torch.isnan(Xb[:GUARD]).all()) and bool(torch.isnan(Xb[GUARD + x_rows:]).all())


# ------------------------------------------------------------------------------------------------ 3. NaN, 4. graphs
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_a_nan_row_of_x_reaches_exactly_the_rows_that_index_it(gpu, gated):
    pkg = gpu
    ty, inf, x_rows = "f16", 128, 60
    rows, width = (96, 48) if gated else (96, 96)
    counts = [20, 70, 0, 33]
    off, tokens = layout(counts, head=2, tail=3)
    G = len(counts)
    rng = np.random.default_rng(4200)
    keep = mask24(rng, G * rows, inf)
    Wn = np.where(keep, rng.uniform(0.25, 2.0, keep.shape) * rng.choice(np.array([-1.0, 1.0]), size=keep.shape), 0.0)
    pr = Problem(pkg, rng, ty, G, rows, inf, tokens, W=Wn)
    Xn = rng.uniform(0.25, 2.0, (x_rows, inf))
    Xn[17, :] = np.nan
    idx = rng.integers(0, x_rows, tokens)
    idx[idx == 17] = 18
    hit = np.array([0, 1, 2, 5, 30, 95, 100, 124, 127])           # unowned rows (0, 1 and the tail) and rows of groups 0, 1 and 3
    idx[hit] = 17
    Xb, X = pr.xbuf(Xn)
    got = pr.run(X, off, width, gated, x_index=idx, x_rows=x_rows, **(dict(act="none") if gated else {}))
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
    ty, inf, tokens, G, x_rows = "bf16", 192, 300, 4, 170
    rows, width = (130, 65) if gated else (77, 77)
    rng = np.random.default_rng(4300)
    pr = Problem(pkg, rng, ty, G, rows, inf, tokens)
    Xb, X = pr.xbuf(rng.uniform(-2, 2, (x_rows, inf)))
    ldy = width + 4
    fn = pkg.linear24_grouped_glu if gated else pkg.linear24_grouped
    call = lambda Y, off, idx: fn(pr.blob, X, Y, off, G, tokens, width, inf, ldx=pr.ldx, ldy=ldy, x_index=idx, x_rows=x_rows)
    routings = [([0, 100, 100, 230, 300], rng.integers(0, x_rows, tokens)), ([10, 11, 140, 141, 290], rng.integers(0, x_rows, tokens))]
    eager = []
    for off, idx in routings:
        Ye = torch.full((tokens, ldy), SENTINEL, dtype=DT[ty], device=DEV)
        call(Ye, i32dev(off), i32dev(idx))
        torch.cuda.synchronize()
        eager.append(Ye)
    assert not torch.equal(bits(eager[0]), bits(eager[1]))
    d_off, d_idx = i32dev(routings[0][0]), i32dev(routings[0][1])
    Y = torch.full((tokens, ldy), SENTINEL, dtype=DT[ty], device=DEV)
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


# ------------------------------------------------------------------------------------------------ 5. the C++ header mirror
def test_cpp_header_mirror(gpu):
    """examples/bin/moe_block: sparsifyme::moe_route, spmma_plan_t::linear_glu_grouped / linear_grouped with x_index, moe_combine on a
    seeded router's ids, against the same block done with a host-side stable sort, a materialised X[x_index], the existing plan calls and
    a host combine; the example checks itself bit for bit and exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "moe_block")
    assert os.path.exists(exe), "examples/bin/moe_block is missing: build() makes it"
    res = subprocess.run([exe, "8", "128", "192", "150", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "equal to the host-routed block bit for bit: yes" in res.stdout
