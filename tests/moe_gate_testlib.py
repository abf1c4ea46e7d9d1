"""Numpy restatements of sm_moe_gate_* (include/sparsifyme.h) shared by tests/test_moe_gate_abi.py and tests/test_gpu_moe_gate.py: the
selection rule, the weights in fp32 to the operation and in fp64, and the bound the GPU test holds the device to."""
import numpy as np

SOFTMAX, SIGMOID = 0, 1
ULP = 2.0 ** -24
F32 = np.float32


def keys(x, scoring=SOFTMAX, bias=None, dtype=np.float64):
    """key_e in `dtype` (float32: the device's operations; float64: the reference the premise of the bias test is stated in); NaN -> -inf"""
    x = np.asarray(x, dtype=dtype)
    if bias is None:
        k = x.copy()
    else:
        assert scoring == SIGMOID
        one = dtype(1)
        with np.errstate(all="ignore"):
            k = (one / (one + np.exp(-x))).astype(dtype) + np.asarray(bias, dtype=dtype)
    return np.where(np.isnan(k), -np.inf, k).astype(dtype)


def select(key, top_k):
    """ids[t][j]: descending key, equal keys in ascending expert index (a stable sort of -key; -0 == +0)"""
    return np.argsort(-np.asarray(key), axis=-1, kind="stable")[..., :top_k].astype(np.int32)


def weights(x, ids, scoring, renorm, scale, dtype=np.float64):
    """The header's weights at the given ids, every operation rounded to `dtype`; the sums over j in ascending j.  x: [tokens][experts]."""
    x = np.asarray(x, dtype=dtype)
    scale = dtype(scale)
    xs = np.take_along_axis(x, ids.astype(np.int64), axis=1)
    one = dtype(1)
    with np.errstate(all="ignore"):
        if scoring == SOFTMAX:
            m = xs[:, :1] if renorm else np.max(x, axis=1, keepdims=True)
            e = np.exp((xs - m).astype(dtype)).astype(dtype)
            if renorm:
                S = np.zeros((x.shape[0], 1), dtype=dtype)
                for j in range(ids.shape[1]):
                    S = (S + e[:, j:j + 1]).astype(dtype)
            else:
                S = np.sum(np.exp((x - m).astype(dtype)).astype(dtype), axis=1, keepdims=True, dtype=dtype)
            return ((e / S).astype(dtype) * scale).astype(dtype)
        q = (one / (one + np.exp(-xs).astype(dtype)).astype(dtype)).astype(dtype)
        if not renorm:
            return (q * scale).astype(dtype)
        S = np.zeros((x.shape[0], 1), dtype=dtype)
        for j in range(ids.shape[1]):
            S = (S + q[:, j:j + 1]).astype(dtype)
        return ((q / S).astype(dtype) * scale).astype(dtype)


def bound_terms(x, experts, top_k, scoring, renorm):
    """(N, D) of the bound (N + D + 11) * 2^-24 per row: N the number of terms in the denominator (top_k; experts for the softmax over all
    experts; none for the sigmoid that is not renormalised), D the row's largest |x - m|, m the row's maximum."""
    x = np.asarray(x, dtype=np.float64)
    D = np.max(np.abs(x - np.max(x, axis=1, keepdims=True)), axis=1, keepdims=True)
    N = top_k if renorm else (experts if scoring == SOFTMAX else 0)
    return N, D


def worst_ratio(w_dev, x, ids, experts, top_k, scoring, renorm, scale):
    """max over the elements of (relative error against the fp64 evaluation at these ids) / bound"""
    want = weights(x, ids, scoring, renorm, scale, np.float64)
    assert np.all(np.isfinite(want)) and np.all(want != 0)
    N, D = bound_terms(x, experts, top_k, scoring, renorm)
    assert float(D.max()) <= 24.0, "the inputs keep D at or below 24"
    rel = np.abs(np.asarray(w_dev, dtype=np.float64) - want) / np.abs(want)
    return float(np.max(rel / ((N + D + 11) * ULP)))

