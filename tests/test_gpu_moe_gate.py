"""sm_moe_gate_{f16,bf16,f32} on the device (-m gpu): the router's logits to top_k ids and fp32 weights in one launch.

Ids are compared bit for bit with the definition's (tests/moe_gate_testlib.py): descending key, equal keys in ascending expert index, a
NaN key as -inf.  Weights are held to the fp64 evaluation of the definition AT THE DEVICE'S OWN IDS within (N + D + 11) * 2^-24 relative:
N the terms of the denominator (top_k; experts for the softmax that is not renormalised; none for the sigmoid that is not), D the row's
largest |x - m| (kept <= 24 by the inputs), 11 = four rounded operations (or three and the roundings of the scale) + 4 ulp for each of the
two device exponentials (an allowance, not a measurement).  Every case prints its worst error as a share of the bound before it asserts.

Every call reads logits at a moved base (an odd element offset into the allocation) with ld > experts and NaN in the padding, and writes
ids and weights that sit between sentinel guard words; every case asks sm_moe_gate_form which form it runs, and runs twice (same bits).
Shapes: tokens 1, 3, 4, 5, 257 (a partial last workgroup of four waves); experts 1, 2, 8, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000,
1024 (every keys-per-lane instantiation, both sides of each boundary, ragged last registers); top_k 1, 2, 8, 32 and top_k == experts."""
import os
import subprocess

import numpy as np
import pytest
import torch
from linear24_testlib import DEV
from moe_route_testlib import route_ref

import moe_gate_testlib as gl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8                  # words before and behind both outputs
BASE, PAD = 5, 3           # the logits start BASE elements into their allocation; ld = experts + PAD
SENT_I, SENT_W = -77777, -12345.0
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
SOFTMAX, SIGMOID = gl.SOFTMAX, gl.SIGMOID
# (scoring, renormalize, scale): both scorings, both renormalisations, both scales
MODES = [(SOFTMAX, True, 1.0), (SOFTMAX, False, 2.5), (SIGMOID, True, 2.5), (SIGMOID, False, 1.0)]
MODE_IDS = ["softmax-renorm", "softmax-all-x2.5", "sigmoid-renorm-x2.5", "sigmoid"]


def form_of(experts):
    return "lane%d" % next(n for n in (1, 2, 4, 8, 16) if n >= -(-experts // 64))


def rounded(x, ty):
    """x rounded to the logit type, as float64 (the exact values the device reads)"""
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).to(TORCH[ty]).to(torch.float64).numpy()


class Gate:
    """One shape's buffers: guarded outputs, the padded logits at a moved base."""

    def __init__(self, pkg, ty, tokens, experts, top_k):
        self.pkg, self.ty, self.tokens, self.experts, self.top_k = pkg, ty, tokens, experts, top_k
        self.ld = experts + PAD
        self.P = tokens * top_k
        self.buf = torch.full((BASE + tokens * self.ld + GUARD,), float("nan"), dtype=TORCH[ty], device=DEV)
        self.logits = self.buf[BASE:BASE + tokens * self.ld]
        self.ibuf = torch.full((self.P + 2 * GUARD,), SENT_I, dtype=torch.int32, device=DEV)
        self.wbuf = torch.full((self.P + 2 * GUARD,), SENT_W, dtype=torch.float32, device=DEV)
        self.ids, self.w = self.ibuf[GUARD:GUARD + self.P], self.wbuf[GUARD:GUARD + self.P]
        assert pkg.moe_gate_form(tokens, experts, top_k) == form_of(experts)

    def load(self, x):
        """x: [tokens][experts], already representable in the logit type"""
        v = self.logits.view(self.tokens, self.ld)
        v[:, :self.experts] = torch.from_numpy(np.ascontiguousarray(x)).to(TORCH[self.ty]).to(DEV)

    def run(self, scoring, renorm, scale, bias=None):
        self.pkg.moe_gate(self.logits, self.ids, self.w, self.tokens, self.experts, self.top_k, scoring=scoring, renormalize=renorm, scale=scale,
                          select_bias=bias, ld=self.ld)

    def outputs(self):
        torch.cuda.synchronize()
        for b, s in ((self.ibuf, SENT_I), (self.wbuf, SENT_W)):
            assert bool((b[:GUARD] == s).all()) and bool((b[GUARD + self.P:] == s).all()), "a guard word of an output was written"
        return (self.ids.cpu().numpy().reshape(self.tokens, self.top_k).copy(), self.w.cpu().numpy().reshape(self.tokens, self.top_k).copy())

    def twice(self, scoring, renorm, scale, bias=None):
        self.ids.fill_(SENT_I)
        self.w.fill_(SENT_W)
        self.run(scoring, renorm, scale, bias)
        ids, w = self.outputs()
        self.ids.fill_(SENT_I)
        self.w.fill_(SENT_W)
        self.run(scoring, renorm, scale, bias)
        ids2, w2 = self.outputs()
        assert np.array_equal(ids, ids2) and np.array_equal(w.view(np.int32), w2.view(np.int32)), "two runs on the same logits differ"
        return ids, w


def check_ids(ids, want, experts):
    assert ids.min() >= 0 and ids.max() < experts and all(len(set(r)) == len(r) for r in ids.tolist()), "ids not distinct or out of range"
    bad = np.argwhere(ids != want)
    assert bad.size == 0, f"ids: first mismatch at token {bad[0][0]}, choice {bad[0][1]}: {ids[tuple(bad[0])]} for {want[tuple(bad[0])]}, {len(bad)} in all"


def check_weights(label, w, x, ids, experts, top_k, scoring, renorm, scale):
    ratio = gl.worst_ratio(w, x, ids, experts, top_k, scoring, renorm, scale)
    print(f"margin moe_gate {label}: worst error {ratio:.3f} of the bound")
    assert ratio <= 1.0, f"{label}: error {ratio:.3f} of the bound (N + D + 11) * 2^-24"


# (tokens, experts, top_k, type): every tokens / experts / top_k value of the docstring at least once, every form in every type
CASES = [(1, 1, 1, "f32"), (3, 2, 2, "f16"), (4, 8, 8, "bf16"), (5, 8, 2, "f32"), (257, 63, 8, "f16"), (5, 64, 32, "bf16"), (4, 64, 1, "f32"),
         (4, 65, 1, "f32"), (3, 128, 8, "bf16"), (5, 65, 32, "f16"), (5, 129, 32, "f16"), (3, 256, 2, "f32"), (1, 256, 8, "bf16"),
         (5, 257, 2, "bf16"), (3, 512, 8, "f16"), (4, 513, 8, "f32"), (257, 1000, 8, "bf16"), (3, 1024, 32, "f32"), (4, 1024, 1, "f16"),
         (257, 8, 2, "f32")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_integer_logits_ties_everywhere(gpu, case):
    """logits from a pool of seven integers: equal keys in every row; the ids are np.argsort(-key, kind="stable")'s, the weights the bound's"""
    tokens, experts, top_k, ty = case
    rng = np.random.default_rng(5000 + CASES.index(case))
    x = rng.integers(-3, 4, (tokens, experts)).astype(np.float64)
    g = Gate(gpu, ty, tokens, experts, top_k)
    g.load(x)
    want = gl.select(gl.keys(x), top_k)
    for (scoring, renorm, scale), name in zip(MODES, MODE_IDS):
        ids, w = g.twice(scoring, renorm, scale)
        check_ids(ids, want, experts)
        check_weights(f"integer {ty} {tokens}x{experts} top-{top_k} {name}", w, x, ids, experts, top_k, scoring, renorm, scale)
        if top_k == 1 and renorm:
            assert np.all(w == np.float32(scale)), "top_k = 1 renormalised is exactly the scale"


@pytest.mark.parametrize("experts,top_k,ty", [(8, 8, "f16"), (65, 8, "f32"), (1000, 32, "bf16")])
def test_equal_descending_and_ascending_rows(gpu, experts, top_k, ty):
    ramp = rounded(-24.0 / 1024 * np.arange(experts), ty)            # D < 24; rounding to the type keeps the order (and makes ties)
    assert np.all(np.diff(ramp) <= 0)
    x = np.stack([np.full(experts, 1.5), ramp, ramp[::-1], np.zeros(experts)])
    x[3, 1::2] = -0.0                                                # -0 == +0: still all equal
    g = Gate(gpu, ty, 4, experts, top_k)
    g.load(x)
    want = gl.select(gl.keys(x), top_k)
    assert want[0].tolist() == list(range(top_k)) == want[3].tolist()
    for (scoring, renorm, scale), name in zip(MODES, MODE_IDS):
        ids, w = g.twice(scoring, renorm, scale)
        check_ids(ids, want, experts)
        check_weights(f"ramps {ty} {experts} top-{top_k} {name}", w, x, ids, experts, top_k, scoring, renorm, scale)


@pytest.mark.parametrize("case", [(5, 8, 2, "f32"), (257, 64, 8, "bf16"), (4, 129, 8, "f32"), (3, 1000, 32, "f16"), (5, 1024, 8, "f32")],
                         ids=lambda c: "x".join(map(str, c)))
def test_random_logits_weights_at_the_devices_ids(gpu, case):
    """logits ~ N(0, 3) clipped to +-12 (D <= 24) and rounded to the type: without a bias the key is the logit itself, so the ids stay exact"""
    tokens, experts, top_k, ty = case
    rng = np.random.default_rng(5100 + experts + top_k)
    x = rounded(np.clip(rng.normal(0.0, 3.0, (tokens, experts)), -12, 12), ty)
    g = Gate(gpu, ty, tokens, experts, top_k)
    g.load(x)
    want = gl.select(gl.keys(x), top_k)
    for (scoring, renorm, scale), name in zip(MODES, MODE_IDS):
        ids, w = g.twice(scoring, renorm, scale)
        check_ids(ids, want, experts)
        check_weights(f"random {ty} {tokens}x{experts} top-{top_k} {name}", w, x, ids, experts, top_k, scoring, renorm, scale)


@pytest.mark.parametrize("experts,top_k,ty", [(8, 8, "f32"), (63, 8, "f16"), (65, 32, "bf16"), (1000, 32, "f32")])
def test_nan_and_inf_rows(gpu, experts, top_k, ty):
    """ids: the rule's (a NaN key as -inf), distinct, in range -- whatever the row holds; weights: NaN exactly where the fp64 evaluation of the
    definition is NaN"""
    rng = np.random.default_rng(5200 + experts)
    tokens = 9
    x = rng.integers(-3, 4, (tokens, experts)).astype(np.float64)
    x[0, :] = np.nan                                                 # nothing but NaN: ids 0 .. top_k - 1
    x[1, :] = -np.inf
    x[2, :] = np.inf
    x[3, rng.random(experts) < 0.5] = np.nan
    x[4, rng.random(experts) < 0.3] = -np.inf
    x[5, experts // 2] = np.inf
    x[6, rng.random(experts) < 0.4] = np.nan
    x[6, rng.random(experts) < 0.3] = np.inf
    x[6, rng.random(experts) < 0.3] = -np.inf
    x[7, experts - 1] = np.nan                                       # one NaN: chosen only when top_k == experts
    x[8, :] = np.where(np.arange(experts) % 2 == 0, np.nan, -np.inf)  # NaN and -inf are EQUAL keys: ascending index
    g = Gate(gpu, ty, tokens, experts, top_k)
    g.load(x)
    want = gl.select(gl.keys(x), top_k)
    assert want[0].tolist() == list(range(top_k)) == want[8].tolist()
    for scoring, renorm, scale in MODES:
        ids, w = g.twice(scoring, renorm, scale)
        check_ids(ids, want, experts)
        ref = gl.weights(x, ids, scoring, renorm, scale, np.float64)
        assert np.array_equal(np.isnan(w), np.isnan(ref)), (scoring, renorm, np.argwhere(np.isnan(w) != np.isnan(ref))[:4].tolist())
        assert np.isnan(ref).any() and not np.isnan(ref).all()


GAP = 2.0 ** -16           # 64 x the fp32 error of q + b (|q + b| < 2: half an ulp is 2^-24 for the add, q itself a few ulp of 2^-24)


def biased_rows(rng, tokens, experts, top_k, ty):
    """logits ~ N(0, 3) in the type, bias uniform in +-0.5; a row is resampled until the fp64 keys of its first top_k + 1 experts (in key
    order) are pairwise at least GAP apart, so that the device's fp32 keys order them the same way.  No row is left out."""
    bias = rng.uniform(-0.5, 0.5, experts).astype(np.float32)
    x = np.empty((tokens, experts))
    resampled = 0
    for t in range(tokens):
        while True:
            x[t] = rounded(np.clip(rng.normal(0.0, 3.0, experts), -12, 12), ty)
            k = np.sort(gl.keys(x[t], SIGMOID, bias))[::-1][:top_k + 1]
            if np.all(-np.diff(k) >= GAP):
                break
            resampled += 1
    return x, bias, resampled


@pytest.mark.parametrize("case", [(5, 8, 2, "f16"), (257, 64, 8, "bf16"), (4, 65, 1, "f32"), (3, 256, 8, "f16"), (5, 1000, 8, "f16"), (3, 1024, 2, "f32"),
                                  (4, 8, 8, "f32")], ids=lambda c: "x".join(map(str, c)))
def test_select_bias_decides_the_ids_not_the_weights(gpu, case):
    tokens, experts, top_k, ty = case
    rng = np.random.default_rng(5300 + experts + top_k)
    x, bias, resampled = biased_rows(rng, tokens, experts, top_k, ty)
    k64 = gl.keys(x, SIGMOID, bias)
    srt = -np.sort(-k64, axis=1)[:, :top_k + 1]
    assert np.all(-np.diff(srt, axis=1) >= GAP), "the premise holds on every row the test uses"
    want = gl.select(k64, top_k)
    assert not np.array_equal(want, gl.select(gl.keys(x), top_k)) or experts == top_k, "the bias changes the selection of this case"
    g = Gate(gpu, ty, tokens, experts, top_k)
    g.load(x)
    d_bias = torch.from_numpy(bias).to(DEV)
    for renorm, scale in ((True, 1.0), (False, 2.5)):
        ids, w = g.twice(SIGMOID, renorm, scale, d_bias)
        check_ids(ids, want, experts)
        check_weights(f"bias {ty} {tokens}x{experts} top-{top_k} renorm={renorm}", w, x, ids, experts, top_k, SIGMOID, renorm, scale)
    print(f"bias {ty} {tokens}x{experts} top-{top_k}: {resampled} rows resampled")


@pytest.mark.parametrize("experts,top_k,ty", [(8, 4, "f32"), (130, 8, "bf16"), (1024, 32, "f16")])
def test_select_bias_exact_ties_fall_to_the_lower_index(gpu, experts, top_k, ty):
    """equal logits and equal biases in pairs (2i, 2i + 1): the fp32 keys of a pair are the same bits; different pairs lie more than GAP apart"""
    half = experts // 2
    vals = rounded(np.linspace(3.0, -3.0, half), ty)
    perm = np.random.default_rng(5400 + experts).permutation(half)
    x = np.repeat(vals[perm], 2)[None, :]
    bias = np.full(experts, 0.25, dtype=np.float32)
    k64 = gl.keys(x, SIGMOID, bias)
    gaps = -np.diff(-np.sort(-k64[0]))
    assert np.all((gaps == 0) | (gaps >= GAP)) and int((gaps == 0).sum()) == half
    want = gl.select(k64, top_k)
    assert np.all(want[0, 0::2] % 2 == 0) and np.all(want[0, 1::2] == want[0, 0::2] + 1)
    g = Gate(gpu, ty, 1, experts, top_k)
    g.load(x)
    ids, w = g.twice(SIGMOID, True, 1.0, torch.from_numpy(bias).to(DEV))
    check_ids(ids, want, experts)
    check_weights(f"bias pairs {ty} {experts} top-{top_k}", w, x, ids, experts, top_k, SIGMOID, True, 1.0)


@pytest.mark.parametrize("ty", ["bf16", "f32"])
def test_hipgraph_gate_then_route_follows_the_logits(gpu, ty):
    """gate -> sm_moe_route captured once (one stream: a chain of kernel nodes); the logits then change in device memory only"""
    pkg, tokens, experts, top_k = gpu, 37, 65, 8
    rng = np.random.default_rng(5500)
    g = Gate(pkg, ty, tokens, experts, top_k)
    Pn = tokens * top_k
    assert pkg.moe_route_form(tokens, top_k, experts) == "single"
    i32 = lambda n: torch.full((n,), SENT_I, dtype=torch.int32, device=DEV)
    off, st, sp, pp = i32(experts + 1), i32(Pn), i32(Pn), i32(Pn)
    logit_sets = [rng.integers(-3, 4, (tokens, experts)).astype(np.float64), rounded(np.clip(rng.normal(0, 3, (tokens, experts)), -12, 12), ty)]

    def block():
        g.run(SOFTMAX, True, 1.0)
        pkg.moe_route(g.ids, tokens, top_k, experts, off, st, sp, pp)

    g.load(logit_sets[0])
    block()                                          # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        block()
    for x in logit_sets + [logit_sets[0]]:
        g.load(x)
        for v in (g.ids, off, st, sp, pp):
            v.fill_(SENT_I)
        g.w.fill_(SENT_W)
        graph.replay()
        ids, w = g.outputs()
        want = gl.select(gl.keys(x), top_k)
        check_ids(ids, want, experts)
        r_off, r_st, r_sp, r_pp = route_ref(want.reshape(-1), top_k, experts)
        assert np.array_equal(off.cpu().numpy(), r_off) and np.array_equal(pp.cpu().numpy(), r_pp) and np.array_equal(st.cpu().numpy(), r_st)
        assert int(r_off[-1]) == Pn
        check_weights(f"graph replay {ty}", w, x, ids, experts, top_k, SOFTMAX, True, 1.0)


def test_cpp_header_mirror(gpu):
    """examples/bin/moe_gate: sparsifyme::moe_gate -> moe_route through the headers; the example checks ids, weights and offsets itself and
    exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "moe_gate")
    assert os.path.exists(exe), "examples/bin/moe_gate is missing: build() makes it"
    for argv in (["64", "300", "8"], ["257", "33", "8", "sigmoid"]):
        res = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.count(": yes") == 3 and "NO" not in res.stdout, res.stdout
