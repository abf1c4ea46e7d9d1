"""What the 1-byte (fp8 e4m3 / e5m2, int8) GPU tests share: the format tables, the bound's constants, bytes <-> values, the operand
generators and the numpy restatement of the per-row quantisation.  numpy only at import time.  ROUND and TINY here are the 1-byte files'
(half an ulp and the smallest subnormal of the OUTPUT type); parity_testlib and linear24_testlib keep constants of the same names with
values of their own."""
import numpy as np

FMTS = ["e4m3", "e5m2"]
PAIRS = [(a, b) for a in FMTS for b in FMTS]
OUTS = ["f32", "f16", "bf16"]
ROUND = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f32": 2.0 ** -149, "f16": 2.0 ** -24, "bf16": 2.0 ** -133}
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
# every byte with a name: +-0, the NaNs, e5m2 +-inf, the largest finite values, subnormals
SPECIALS = {"e4m3": [0x00, 0x80, 0x7f, 0xff, 0x7e, 0xfe, 0x01, 0x81, 0x07, 0x08, 0x38, 0xb8],
            "e5m2": [0x00, 0x80, 0x7c, 0xfc, 0x7d, 0x7e, 0x7f, 0xfd, 0xfe, 0xff, 0x7b, 0x01, 0x83, 0x04, 0x3c, 0xbc]}
EXACT_VALS = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0], dtype=np.float32)


# the fp32 accumulation term of the bound counts the products the instructions sum: k rounded up to whole 128-k steps (the
# padding products are zeros, but a k = 64 product is one 128-k instruction, and its error is that of one: measured 1.15x
# over a bound with k = 64 itself, for the sparse instruction as for the dense one)
def ksteps(k):
    return (k + 127) // 128 * 128


def tdt(f):
    import torch
    return {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[f]


def odt(o):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[o]


def dev8(a, f):
    """uint8 numpy bytes -> fp8 device tensor of format f."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).view(tdt(f)).cuda()


def bytes_of(t):
    import torch
    return t.view(torch.uint8).cpu().numpy()


def img16(a, f):
    """the fp16 image's bit patterns (uint16) of fp8 bytes a."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).view(tdt(f)).to(torch.float16).view(torch.int16).numpy().view(np.uint16)


# Two ways to the fp64 values of fp8 bytes, kept apart because their bodies differ: through the fp16 image (what the 2:4 rules are
# stated on) and by torch's own conversion (the dense GEMM's tests).
def val64(a, f):
    return img16(a, f).view(np.float16).astype(np.float64)


def val64_direct(a, f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).view(tdt(f)).to(torch.float64).numpy()


def to8(x, f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt(f)).view(torch.uint8).numpy().copy()


def finite_bytes(rng, size, f, lo=-2.0, hi=2.0):
    """random finite fp8 values (uniform before rounding) as bytes"""
    return to8(rng.uniform(lo, hi, size), f)


def map_back(pruned16, image16, a):
    """bytes of a where the pruned image kept the element, 0x00 where it dropped it."""
    return np.where(pruned16 == image16, a, 0).astype(np.uint8)


def make_bytes(rng, size, f, kind):
    if kind == "rand":
        return rng.integers(0, 256, size).astype(np.uint8)
    if kind == "ties":  # few distinct magnitudes, both signs, both zeros: ties decided by the lower k
        return rng.choice(np.array([0x00, 0x80, 0x38, 0xb8, 0x40, 0xc0, 0x3c, 0xbc] if f == "e5m2" else [0x00, 0x80, 0x38, 0xb8, 0x40, 0xc0, 0x30, 0xb0],
                                   dtype=np.uint8), size)
    a = rng.integers(0, 256, size).astype(np.uint8)
    sel = rng.random(size) < 0.5
    a[sel] = rng.choice(np.array(SPECIALS[f], dtype=np.uint8), int(sel.sum()))
    return a


# ---------------------------------------------------------------------------------------------
# the per-row quantisation rule of tests/test_gpu_quant_fp8.py's docstring, in numpy
# ---------------------------------------------------------------------------------------------
def nonfinite_bytes(x, q, f):
    """the explicit select of the rule on the SOURCE values x (fp32, exact images of the 16-bit elements)."""
    q = q.copy()
    q[np.isnan(x)] = 0x7F
    inf = np.isinf(x)
    q[inf] = 0x7F if f == "e4m3" else np.where(np.signbit(x[inf]), 0xFC, 0x7C).astype(np.uint8)
    return q


def cast8(y, f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(tdt(f)).view(torch.uint8).numpy()


def ref_quant_rows(x, f):
    """x: rows x k float32 (the exact values of the 16-bit A) -> (Q bytes rows x k, row_scale float32)."""
    fm = np.float32(FMAX[f])
    fin = np.isfinite(x)
    amax = np.maximum(np.where(fin, np.abs(x), np.float32(0)).max(axis=1), np.float32(2.0 ** -100)).astype(np.float32)
    scale = (amax / fm).astype(np.float32)
    inv = (fm / amax).astype(np.float32)
    y = (np.where(fin, x, np.float32(0)) * inv[:, None]).astype(np.float32)
    return nonfinite_bytes(x, cast8(y, f), f), scale
