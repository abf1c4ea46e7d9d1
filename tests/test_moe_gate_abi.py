"""The MoE gate (sm_moe_gate_{f16,bf16,f32}, sm_moe_gate_form) without a GPU: the four symbols are declared, exported and bound with the
header's arity and the #defines match the Python constants; every status is returned before any device work (fake pointers, never
dereferenced), in the order the header states and with a text that names the entry point and the limit; sm_moe_gate_form at both sides
of every keys-per-lane boundary; and the numpy restatement of the definition the GPU test uses (tests/moe_gate_testlib.py) -- fp32 to the
operation against fp64, and against torch.topk / torch.softmax / torch.sigmoid on the CPU on tie-free rows."""
import ctypes
import os
import re

import numpy as np
import pytest

import moe_gate_testlib as gl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
P = ctypes.c_void_p(0x1000)       # stand-in for a device pointer
BIG = 1 << 31
LIM = BIG - 1
MAXG, MAXK = 1024, 32
GATES = ["sm_moe_gate_f16", "sm_moe_gate_bf16", "sm_moe_gate_f32"]
WHO = b"sm_moe_gate_{f16,bf16,f32}"


def _err(pkg):
    return pkg.lib().sm_last_error()


def gate(pkg, name="sm_moe_gate_f32", logits=P, bias=None, ids=P, w=P, tokens=8, experts=16, top_k=2, ld=None, scoring=0, renorm=1, scale=1.0):
    return getattr(pkg.lib(), name)(logits, bias, ids, w, tokens, experts, top_k, experts if ld is None else ld, scoring, renorm, scale, None)


def gate_form(pkg, tokens, experts, top_k):
    f = ctypes.c_int(-1)
    assert pkg.lib().sm_moe_gate_form(tokens, experts, top_k, ctypes.byref(f)) == 0
    assert pkg.moe_gate_form(tokens, experts, top_k) == pkg.MOE_GATE_FORMS[f.value]
    return pkg.MOE_GATE_FORMS[f.value]


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in GATES + ["sm_moe_gate_form"]:
        assert name + "(" in header and name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    sz, ci, cf, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    for name in GATES:
        assert pkg._SIGS[name] == [vp] * 4 + [sz] * 4 + [ci, ci, cf, vp], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(proto.split(",")) == 12 == len(pkg._SIGS[name])
        assert re.search(r"const void\* logits,\s*const float\* select_bias,\s*int\* topk_ids,\s*float\* topk_weights,\s*size_t tokens,\s*size_t experts,"
                         r"\s*size_t top_k,\s*size_t ld,\s*int scoring,\s*int renormalize,\s*float scale,\s*sm_stream_t stream", proto), name
    assert pkg._SIGS["sm_moe_gate_form"][:3] == [sz] * 3 and len(pkg._SIGS["sm_moe_gate_form"]) == 4
    assert len(re.search(r"sm_moe_gate_form\(([^;]*?)\);", header, flags=re.S).group(1).split(",")) == 4
    for k, v in (("SM_MOE_SCORE_SOFTMAX", 0), ("SM_MOE_SCORE_SIGMOID", 1), ("SM_MOE_GATE_MAX_TOP_K", MAXK), ("SM_MOE_GATE_FORM_INVALID", 0),
                 ("SM_MOE_GATE_FORM_EMPTY", 1), ("SM_MOE_GATE_FORM_LANE1", 2), ("SM_MOE_GATE_FORM_LANE2", 3), ("SM_MOE_GATE_FORM_LANE4", 4),
                 ("SM_MOE_GATE_FORM_LANE8", 5), ("SM_MOE_GATE_FORM_LANE16", 6), ("SM_LINEAR24_MAX_GROUPS", MAXG)):
        assert re.search(r"#define %s %d\b" % (k, v), header), k
    assert pkg.MOE_GATE_FORMS == ("invalid", "empty", "lane1", "lane2", "lane4", "lane8", "lane16")
    assert (pkg.MOE_SCORE_SOFTMAX, pkg.MOE_SCORE_SIGMOID, pkg.MOE_GATE_MAX_TOP_K) == (0, 1, MAXK)
    assert callable(pkg.moe_gate) and callable(pkg.moe_gate_form)


@pytest.mark.parametrize("name", GATES)
def test_statuses_before_any_device_work_in_the_stated_order(pkg, name):
    call = lambda **kw: gate(pkg, name, **kw)
    # 1. invalid values
    for kw in (dict(logits=None), dict(ids=None), dict(w=None), dict(ld=15), dict(top_k=17), dict(scoring=2), dict(scoring=-1),
               dict(bias=P, scoring=0), dict(experts=0, ld=0, top_k=1)):
        assert call(**kw) == INVALID, kw
        assert WHO + b": invalid argument" in _err(pkg), kw
    # ... answered before every not-supported shape
    assert call(logits=None, tokens=BIG) == INVALID and call(ids=None, experts=MAXG + 1, ld=MAXG + 1) == INVALID
    assert call(top_k=MAXK + 1, experts=MAXK) == INVALID and call(scoring=7, top_k=MAXK + 1, experts=64) == INVALID
    assert call(ld=BIG - 1, experts=BIG, top_k=1) == INVALID
    # 2. a product or a dimension past 2^31 - 1 ...
    for kw in (dict(tokens=BIG), dict(tokens=1 << 40), dict(tokens=1 << 27, top_k=16), dict(tokens=1 << 16, ld=1 << 15), dict(ld=BIG),
               dict(experts=BIG, ld=BIG, top_k=1), dict(experts=1 << 40, ld=1 << 40, top_k=1 << 39), dict(tokens=1 << 62, ld=1 << 62)):
        assert call(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"2^31-1" in _err(pkg), kw
    # ... before the expert limit, before the top_k limit
    assert call(tokens=BIG, experts=MAXG + 1, ld=MAXG + 1) == NOT_SUPPORTED and b"2^31-1" in _err(pkg)
    for kw in (dict(experts=MAXG + 1, ld=MAXG + 1), dict(experts=MAXG + 1, ld=MAXG + 1, top_k=MAXK + 1), dict(experts=1 << 20, ld=1 << 20)):
        assert call(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"SM_LINEAR24_MAX_GROUPS" in _err(pkg) and b"SM_MOE_GATE_MAX_TOP_K" not in _err(pkg), kw
    for kw in (dict(experts=64, ld=64, top_k=MAXK + 1), dict(experts=MAXG, ld=MAXG, top_k=MAXG)):
        assert call(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"SM_MOE_GATE_MAX_TOP_K" in _err(pkg), kw
    # 3. a zero extent: success, nothing enqueued (the fake pointers never reach a launch) -- but only behind the checks above
    for kw in (dict(tokens=0), dict(top_k=0), dict(tokens=0, top_k=0), dict(tokens=0, bias=P, scoring=1), dict(top_k=0, experts=0, ld=0),
               dict(tokens=0, experts=MAXG, ld=MAXG, top_k=MAXK), dict(top_k=0, tokens=LIM // 16)):
        assert call(**kw) == 0, kw
    assert call(tokens=0, logits=None) == INVALID and call(top_k=0, scoring=2) == INVALID and call(tokens=0, bias=P) == INVALID
    assert call(tokens=0, experts=MAXG + 1, ld=MAXG + 1) == NOT_SUPPORTED and call(tokens=0, experts=64, top_k=MAXK + 1) == NOT_SUPPORTED
    assert call(top_k=0, tokens=BIG) == NOT_SUPPORTED


def test_form_at_both_sides_of_every_keys_per_lane_boundary(pkg):
    assert pkg.lib().sm_moe_gate_form(8, 16, 2, None) == INVALID and b"sm_moe_gate_form" in _err(pkg)
    for below, form_below, form_above in ((64, "lane1", "lane2"), (128, "lane2", "lane4"), (256, "lane4", "lane8"), (512, "lane8", "lane16")):
        for tokens, top_k in ((1, 1), (300, 8), (LIM // 32, 32)):
            assert gate_form(pkg, tokens, below, top_k) == form_below and gate_form(pkg, tokens, below + 1, top_k) == form_above, (below, tokens, top_k)
    assert gate_form(pkg, 5, 1024, 8) == "lane16" and gate_form(pkg, 5, 1025, 8) == "invalid"
    assert gate_form(pkg, 5, 1, 1) == "lane1" and gate_form(pkg, 5, 65, 65 - 33) == "lane2" and gate_form(pkg, 5, 513, 1) == "lane16"
    # the rule over a grid of shapes
    def rule(tokens, experts, top_k):
        if top_k > experts or experts > MAXG or top_k > MAXK or tokens > LIM or tokens * top_k > LIM:
            return "invalid"
        if tokens == 0 or top_k == 0:
            return "empty"
        kpl = -(-experts // 64)
        return "lane%d" % next(n for n in (1, 2, 4, 8, 16) if n >= kpl)
    seen = set()
    for tokens in (0, 1, 4, 257, 1 << 20, LIM // 8, LIM // 8 + 1, LIM, BIG):
        for experts in (0, 1, 8, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024, 1025):
            for top_k in (0, 1, 2, 8, 32, 33):
                assert gate_form(pkg, tokens, experts, top_k) == rule(tokens, experts, top_k), (tokens, experts, top_k)
                seen.add(rule(tokens, experts, top_k))
    assert seen == set(pkg.MOE_GATE_FORMS)
    assert gate_form(pkg, 0, 8, 2) == "empty" and gate_form(pkg, 8, 8, 0) == "empty" and gate_form(pkg, 0, 0, 0) == "empty"
    assert gate_form(pkg, 8, 8, 9) == "invalid" and gate_form(pkg, 1 << 62, 8, 1 << 62) == "invalid" and gate_form(pkg, 1 << 27, 64, 16) == "invalid"


# ------------------------------------------------------------------------------------------------ the numpy restatement
def tie_free_rows(rng, tokens, experts, sigma=3.0):
    """fp32 logits ~ N(0, sigma) clipped to +-12, every row resampled until no two of its values are equal"""
    x = np.clip(rng.normal(0.0, sigma, (tokens, experts)), -12, 12).astype(np.float32)
    for t in range(tokens):
        while len(np.unique(x[t])) != experts:
            x[t] = np.clip(rng.normal(0.0, sigma, experts), -12, 12).astype(np.float32)
    return x


@pytest.mark.parametrize("experts,top_k", [(8, 2), (64, 8), (1024, 8), (1024, 32), (5, 5), (1, 1)])
def test_restatement_in_fp32_against_fp64_and_torch(pkg, experts, top_k):
    import torch
    assert (gl.SOFTMAX, gl.SIGMOID) == (pkg.MOE_SCORE_SOFTMAX, pkg.MOE_SCORE_SIGMOID)   # the restatement speaks the package's scoring codes
    rng = np.random.default_rng(40 + experts + top_k)
    tokens = 40
    x = tie_free_rows(rng, tokens, experts)
    ids = gl.select(gl.keys(x, dtype=np.float32), top_k)
    assert np.array_equal(ids, gl.select(gl.keys(x, dtype=np.float64), top_k))          # no exp decides an id: fp32 exact -> fp64
    tx = torch.from_numpy(x)
    t_ids = torch.topk(tx, top_k, dim=1).indices.numpy()
    assert np.array_equal(ids, t_ids)                                                   # tie-free rows: torch.topk's order is the rule's
    assert all(len(set(r)) == top_k for r in ids.tolist()) and ids.min() >= 0 and ids.max() < experts
    for scoring, renorm, scale in ((0, True, 1.0), (0, False, 1.0), (0, True, 2.5), (1, True, 1.0), (1, False, 2.5)):
        w32 = gl.weights(x, ids, scoring, renorm, scale, np.float32)
        assert w32.dtype == np.float32
        ratio = gl.worst_ratio(w32, x, ids, experts, top_k, scoring, renorm, scale)
        assert ratio <= 1.0, (scoring, renorm, scale, ratio)                            # the restatement itself is inside the device's bound
        score = torch.softmax(tx.double(), dim=1) if scoring == 0 else torch.sigmoid(tx.double())
        tw = torch.gather(score, 1, torch.from_numpy(t_ids.astype(np.int64)))
        if renorm:
            tw = tw / tw.sum(dim=1, keepdim=True)
        tw = (tw * scale).numpy()
        assert np.allclose(w32, tw, rtol=1e-5, atol=0), (scoring, renorm, scale)
    if top_k == 1:
        assert np.all(gl.weights(x, ids, 0, True, 2.5, np.float32) == np.float32(2.5))  # e / e = 1 exactly, times scale
        assert np.all(gl.weights(x, ids, 1, True, 2.5, np.float32) == np.float32(2.5))


def test_restatement_ties_nan_and_bias(pkg):
    assert (gl.SOFTMAX, gl.SIGMOID) == (pkg.MOE_SCORE_SOFTMAX, pkg.MOE_SCORE_SIGMOID)
    # equal keys in ascending expert index; -0 == +0; NaN as -inf behind every number, among themselves by index
    x = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, np.nan, -np.inf, np.nan, 3.0]])
    assert gl.select(gl.keys(x), 9).tolist() == [[1, 2, 8, 0, 3, 4, 5, 6, 7]]
    assert gl.select(gl.keys(np.zeros((2, 6))), 4).tolist() == [[0, 1, 2, 3]] * 2
    # the bias decides the ids, never the weights
    x = np.array([[2.0, 1.0, 0.0, -1.0]])
    b = np.array([0.0, 0.0, 0.9, 0.0], dtype=np.float32)
    ids = gl.select(gl.keys(x, gl.SIGMOID, b), 2)
    assert ids.tolist() == [[2, 0]]
    w = gl.weights(x, ids, gl.SIGMOID, False, 1.0)
    assert np.allclose(w, [[0.5, 1 / (1 + np.exp(-2.0))]])
    # NaN where IEEE puts it: a selected NaN, or inf - inf
    w = gl.weights(np.array([[np.nan, 1.0, 0.0]]), np.array([[1, 2, 0]], dtype=np.int32), gl.SOFTMAX, True, 1.0)
    assert np.all(np.isnan(w))
    w = gl.weights(np.array([[np.inf, 1.0, 0.0]]), np.array([[0, 1]], dtype=np.int32), gl.SOFTMAX, True, 1.0)
    assert np.all(np.isnan(w))
    w = gl.weights(np.array([[-np.inf, 1.0, 0.0]]), np.array([[1, 2, 0]], dtype=np.int32), gl.SOFTMAX, True, 1.0)
    assert not np.any(np.isnan(w)) and w[0, 2] == 0
