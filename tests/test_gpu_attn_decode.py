"""sm_attn_decode_{f16,bf16} on the device (-m gpu): single-query attention over a paged KV cache, grouped query heads, split along the context.

Every case (tests/attn_decode_testlib.py: CASES) reads its operands at moved bases with pitches above their extents and the type's NaN in all
padding, in every slot at or beyond L of a sequence's last page, in every page no table refers to and in a guard page in front of page 0 and
behind the last page -- the pages an UNCLAMPED kernel would address from the absent ids -1 and num_pages, which the table holds inside the live
range of some sequences and in every column at or beyond ceil(L / page_size): a wrong kernel shows NaN, it does not fault.  O, lse and the
workspace sit between sentinel words and the workspace is exactly the reported size; each case asserts its form through the query, runs twice
(same bits) and checks that no input and nothing outside the outputs changed.  Page tables are permuted and not monotone.

One-hot class (addressing, bit for bit): scale = 1, q has 8 entries of 4 (|q|^2 = 128) on a support of its own inside its group, K is zero
except K[target] += q, so the target scores 128, every other token 0 and p is exactly one-hot (exp2f(-128 log2e) = 0 in fp32; the premise is
asserted); V's bits encode (page, slot, kv head, dim); O is V's target row bit for bit and lse = 128.  Targets differ per (sequence, query head):
the first and the last token, the last slot of a page and the first of the next, the last token of a chunk and the first of the next.
Uniform class (reduction and combine, bit for bit): Q = 0, so every p = 1 and every w_c = 1; V integers with |v| <= 7 (7 L < 2^24: every partial
sum is an exact integer in any order; asserted); O = rne16(fp32(sum v) / fp32(T)) bit for bit and lse = logf(T) within 2 ulp.
General data: Q, K ~ N(0, 1), V ~ N(0, sigma), sigma 0.01 / 1 / 30, scale = head_dim^-1/2, and 8 times that (a peaked softmax); O against the
fp64 definition at the device's inputs within, per element,
    1/2 ulp16 at max(|ref|, |O|) + (2 u + 2 delta + (T + head_dim + 16) 2^-24) A,
u the unit roundoff of the 16-bit type (a p_t that rounds to the other neighbour on the device moves numerator and denominator by at most
u p_t each), delta = (head_dim + 2) 2^-24 scale max_t sum_d |q_d k_t,d| (the fp32 scores move every p by a factor e^(+-delta), above and below
the division), T the present tokens (the two fp32 sums in any order), head_dim + 16 for exp2f, the combine and the division, A = sum_t p_t
|v_t,d| / sum_t p_t in fp64: an allowance derived from the definition, not a measurement (tests/test_attn_decode_abi.py holds the fp32
restatement to it on these same cases without a device).  lse is held to delta + 8 2^-24 max(1, |lse|).  Every case prints its worst error
as a share of the bound before it asserts.

Which failure each shape of the table is the smallest to catch -- L = 1: a kernel that needs a full tile or reads slot 1; 15 / 16 / 17: the edge
of a 16-token matrix-instruction tile; page_size -+ 1: the last slot of a page, the first of the next, a second table column; L = 0 among live
sequences: the +0 / -inf path and a workgroup that returns at once; max_pages * page_size = CHUNK and CHUNK - 1 / CHUNK: the largest DIRECT
shape and a full last wave; CHUNK + 1: the smallest SPLIT, a second chunk of one token; 2 CHUNK + 3, 5 CHUNK: more chunks than waves, the
ascending combine, stale workspace records of shorter sequences; page 128 with CHUNK 256: pages longer than a wave's 64 tokens; group 1, 2, 4 (the
4-row class, rows beyond the group zero-padded), 5 (the 16-row class, odd), 8, 16 (every row of the tile); kv_heads 2, 3: the head's column
offset in a token row; head_dim 64: two matrix instructions per tile and 8 lanes per V row; an absent page as a chunk's only page: (-inf, 0, 0)
through the combine; every page absent: +0 and -inf from live lengths; seq_lens above the capacity and negative: the clamp; shared prefix pages:
two sequences reading one page."""
import os
import subprocess

import numpy as np
import pytest
import torch

import attn_decode_testlib as al
import guard_testlib as gl
import parity_testlib as pl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_margin_report = gl.margin_report_fixture("attn_decode: worst error / bound of {n} comparisons (O and lse of every general-data case), worst first")


def problem(pkg, case, what):
    rng = np.random.default_rng(al.seed(al.SALT, what, al.CASES.index(case)))
    return al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng), rng


@pytest.mark.parametrize("case", al.CASES, ids=al.case_id)
def test_one_hot_class_bit_for_bit(gpu, case):
    pr, rng = problem(gpu, case, "exact")
    Q, K, V, targets, want, wl = al.one_hot(pr, rng)
    ob, lse = al.Layout(pr, Q, K, V, torch).twice(gpu, 1.0, al.form_of(pr))
    bad = np.argwhere(ob != want)
    assert bad.size == 0, f"O is not V's target row at (sequence, head, dim) {bad[:4].tolist()}; targets (page, slot, token) {[targets.get((b[0], b[1])) for b in bad[:4]]}"
    assert np.array_equal(lse, wl), "lse is not 128 (-inf for a sequence without a present token)"


@pytest.mark.parametrize("case", al.CASES, ids=al.case_id)
def test_uniform_class_bit_for_bit(gpu, case):
    pr, rng = problem(gpu, case, "uniform")
    Q, K, V, want, wl = al.uniform(pr, rng)
    ob, lse = al.Layout(pr, Q, K, V, torch).twice(gpu, pr.hd ** -0.5, al.form_of(pr))
    bad = np.argwhere(ob != want)
    assert bad.size == 0, f"O is not rne16(sum v / T) at (sequence, head, dim) {bad[:4].tolist()}: {ob[tuple(bad[0])]:#x} for {want[tuple(bad[0])]:#x}"
    fin = np.isfinite(wl)
    assert np.array_equal(np.isneginf(lse), ~fin), "lse = -inf exactly where no token is present"
    assert np.all(np.abs(lse[fin].astype(np.float64) - wl[fin]) <= 2 * np.spacing(np.abs(wl[fin]).astype(np.float32))), "lse is not logf(T) within 2 ulp"
    for s in range(pr.seqs):
        if pr.tokens(s)[0].size == 0:
            assert not ob[s].any(), "no present token: O = +0"


@pytest.mark.parametrize("case", al.CASES, ids=al.case_id)
def test_general_data_within_the_bound(gpu, case):
    pr, rng = problem(gpu, case, "general")
    for sigma, mult in ((0.01, 1.0), (1.0, 1.0), (30.0, 1.0), (1.0, 8.0)):
        Q, K, V = al.general(pr, rng, sigma)
        scale = mult * pr.hd ** -0.5
        ob, lse = al.Layout(pr, Q, K, V, torch).twice(gpu, scale, al.form_of(pr))
        ro, rl = al.worst_ratios(pr, ob, lse, Q, K, V, scale)
        what = f"{al.case_id(case)} sigma {sigma:g} scale x{mult:g} {al.form_of(pr)}"
        print(f"margin attn_decode {what}: O {ro:.3f}, lse {rl:.3f} of the bound")
        pl.MARGINS.append((f"attn_decode O {what}", ro))
        pl.MARGINS.append((f"attn_decode lse {what}", rl))
        assert ro <= 1.0, f"O: error {ro:.3f} of the bound"
        assert rl <= 1.0, f"lse: error {rl:.3f} of the bound"


@pytest.mark.parametrize("ty,hd,group,kvh,ps", [("bf16", 128, 4, 2, 16), ("f16", 64, 8, 1, 32), ("bf16", 128, 16, 1, 128)])
def test_a_sequence_alone_equals_the_sequence_among_five(gpu, ty, hd, group, kvh, ps):
    """the same table row at batch position 3 of 5 and alone: the same bits (the chunk does not depend on seqs)"""
    five = al.case(ty, hd, group, kvh, ps, ["17", "C+1", "P-1", "2*C+3", "C"], "2*C//P+1")
    rng = np.random.default_rng(al.seed(al.SALT, "alone", hd, group, ps))
    pr5 = al.Problem(five, gpu.ATTN_DECODE_CHUNK, rng)
    Q, K, V = al.general(pr5, rng, 1.0)
    o5, l5 = al.Layout(pr5, Q, K, V, torch).twice(gpu, hd ** -0.5, "split")
    for s in (3, 1, 0):
        one = al.Problem(al.case(ty, hd, group, kvh, ps, [five["lens"][s]], five["max_pages"]), gpu.ATTN_DECODE_CHUNK, np.random.default_rng(1))
        one.num_pages, one.table = pr5.num_pages, pr5.table[s:s + 1].copy()
        o1, l1 = al.Layout(one, Q[s:s + 1], K, V, torch).twice(gpu, hd ** -0.5, "split")
        assert np.array_equal(o1[0], o5[s]) and np.array_equal(l1[0].view(np.uint32), l5[s].view(np.uint32)), f"sequence {s} depends on the sequences that ride along"


@pytest.mark.parametrize("ty,hd,group", [("bf16", 128, 4), ("f16", 64, 8)])
def test_hipgraph_replay_after_lengths_and_table_changed_on_the_device(gpu, ty, hd, group):
    """a SPLIT-form call captured once; seq_lens grow past a page and a chunk boundary and block_table rows are rewritten ON THE DEVICE between
    replays; each replay equals the eager call on the new state bit for bit"""
    pkg, C, ps, kvh, seqs = gpu, gpu.ATTN_DECODE_CHUNK, 16, 2, 3
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    max_pages, qh = 3 * C // ps, group * kvh
    num_pages = seqs * max_pages
    assert pkg.attn_decode_form(seqs, qh, kvh, hd, ps, max_pages) == "split"
    rng = np.random.default_rng(al.seed(al.SALT, "graph", hd))
    t16 = lambda a: torch.from_numpy(al.bits_of(a, ty).view(np.int16)).cuda().view(dt)
    q, k, v = t16(rng.normal(0, 1, (seqs, qh, hd))), t16(rng.normal(0, 1, (num_pages, ps, kvh, hd))), t16(rng.normal(0, 1, (num_pages, ps, kvh, hd)))
    tables = [torch.from_numpy(rng.permutation(num_pages).astype(np.int32).reshape(seqs, max_pages)).cuda() for _ in range(2)]
    states = [([ps - 1, C - 1, 5], 0), ([ps + 1, C + 1, 2 * C + 3], 0), ([ps + 1, C + 1, 2 * C + 3], 1), ([3 * C, 1, 0], 1)]
    bt, sl = tables[0].clone(), torch.zeros(seqs, dtype=torch.int32, device="cuda")
    out, lse = torch.zeros((seqs, qh, hd), dtype=dt, device="cuda"), torch.zeros((seqs, qh), dtype=torch.float32, device="cuda")
    ws = torch.zeros(pkg.attn_decode_workspace_size(seqs, qh, hd, ps, max_pages), dtype=torch.uint8, device="cuda")
    sl.copy_(torch.tensor(states[0][0], dtype=torch.int32))
    pkg.attn_decode(q, k, v, bt, sl, out=out, lse=lse, workspace=ws)                      # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pkg.attn_decode(q, k, v, bt, sl, out=out, lse=lse, workspace=ws)
    for lens, which in states:
        sl.copy_(torch.tensor(lens, dtype=torch.int32).cuda())
        bt.copy_(tables[which])
        out.fill_(7.0)
        lse.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eo, el = torch.zeros_like(out), torch.zeros_like(lse)
        pkg.attn_decode(q, k, v, bt, sl, out=eo, lse=el)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eo.view(torch.int16)) and torch.equal(lse.view(torch.int32), el.view(torch.int32)), (lens, which)
        assert bool(torch.isfinite(out.float()).all()) and float(out[0].float().abs().max()) > 0


def test_cpp_header_mirror(gpu):
    """examples/bin/attn_decode: sparsifyme::attn_decode over a permuted page table through the headers; the example checks both exact classes
    on the host and general data against a host fp64 evaluation and exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "attn_decode")
    assert os.path.exists(exe), "examples/bin/attn_decode is missing: build() makes it"
    for argv in (["3", "8", "2", "128", "700"], ["2", "4", "4", "64", "100"]):
        res = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.count(": yes") == 3 and "NO" not in res.stdout, res.stdout
