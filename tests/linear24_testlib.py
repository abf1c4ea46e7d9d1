"""What the GPU tests of the token-major 2:4 linear layers (test_gpu_linear24*.py, test_gpu_moe_*.py) share: a constant or helper is
here when two or more of those files defined it word for word and no second group of them defined it otherwise.  A file whose own
definition differs keeps it and does not import the name; helpers with several variants (bits, compress, i32dev, the Problem classes,
run_* / ref_*, the margin reports and their per-file MARGINS) stay in their files.  Nothing here holds state."""
import numpy as np
import torch

DEV = "cuda:0"
SENTINEL = 7.0
GUARD = 4          # rows before and behind the tokens, inside the allocation
CUS = 256          # the constant the 16-bit layers ask the rule with
BN = {"tile64": 64, "tile128x64": 64, "tile128": 128}

# ---- the 16-bit layers
TYPES = ["f16", "bf16"]
DT = {"f16": torch.float16, "bf16": torch.bfloat16}

# ---- the fp8 layers
FMTS = ["e4m3", "e5m2"]
PAIRS = [(w, x) for w in FMTS for x in FMTS]          # (W's format, X's format)
OUTS = ["f32", "f16", "bf16"]
TDT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
ODT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ROUND = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f32": 2.0 ** -149, "f16": 2.0 ** -24, "bf16": 2.0 ** -133}
NAN_BYTE = {"e4m3": 0x7F, "e5m2": 0x7E}
# fp32 operations between the accumulator and the one rounding, for the widest activation (hardswish), each at most half an ulp of a
# value no larger than S: alpha * w_scale (1), * x_scale (2), s * acc (3), beta * R (4), their sum (5; the two are one fused step when
# contracted), + bias (6), x + 3 (7), x * t (8), the rounded constant 1/6 (9) and the multiply by it (10).  The clamps are exact.  (The gated layer's bound takes the same figure; 3 of them apply there: both
# scales, the bias.)
U_OPS = 10


def _lut(fmt):
    b = np.arange(256)
    sign = np.where(b & 0x80, -1.0, 1.0)
    if fmt == "e4m3":
        e, m = (b >> 3) & 15, b & 7
        v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10))
        v = np.where((e == 15) & (m == 7), np.nan, v)
    else:
        e, m = (b >> 2) & 31, b & 3
        v = np.where(e == 0, m * 2.0 ** -16, (4 + m) * 2.0 ** (e.astype(np.float64) - 17))
        v = np.where(e == 31, np.where(m == 0, np.inf, np.nan), v)
    return sign * v


LUT = {f: _lut(f) for f in FMTS}


def decode8(a, fmt):
    """fp8 bytes -> fp64 values (the tests' own statement of the two OCP encodings)."""
    return LUT[fmt][np.asarray(a, dtype=np.uint8)]


def encode8(x, fmt):
    """fp32 values -> fp8 bytes, rounded to nearest even (what a caller's cast does)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TDT[fmt]).view(torch.uint8).numpy().copy()


def dev8(a, fmt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV).view(TDT[fmt])


# ---- operands
def f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def todev(a, ty):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[ty]).to(DEV)


def mask24(rng, rows, inf):
    keep = np.argsort(rng.random((rows, inf // 4, 4)), axis=2)[:, :, :2]
    m = np.zeros((rows, inf // 4, 4), dtype=bool)
    np.put_along_axis(m, keep, True, axis=2)
    return m.reshape(rows, inf)


# ---- the gated layers: shapes and the gate in fp64
SHAPES = [  # tokens, hidden, in, the form
    (17, 32, 64, "tile64"), (200, 164, 192, "tile64"), (77, 65, 256, "tile64"),      # 65: odd hidden, the up block starts at an odd row
    (260, 4099, 128, "tile128x64"), (260, 4100, 192, "tile128x64"),
    (300, 8195, 128, "tile128"), (300, 8196, 192, "tile128"),
    (1, 16, 64, "decode"), (9, 1011, 192, "decode"), (16, 8192, 64, "decode"),       # 8192: on the limit
    (5, 40, 4160, "decode"),                                                         # 65 stages: a second trip round the K loop (fp8: odd tail)
    (16, 8193, 64, "tile64"),                                                        # a tile form at <= 16 tokens
]
SID = lambda s: "x".join(map(str, s[:3]))
INT_SHAPES = [(17, 32, "tile64"), (77, 65, "tile64"), (260, 4099, "tile128x64"), (300, 8195, "tile128"), (1, 16, "decode"), (9, 1011, "decode"),
              (16, 8192, "decode"), (16, 8193, "tile64")]


def silu64(g):
    with np.errstate(over="ignore", invalid="ignore"):
        return g / (1.0 + np.exp(-g))


def act64(g, act):
    if act == "relu":
        return np.maximum(g, 0.0)
    return silu64(g) if act == "silu" else g


# ---- the grouped and gathered layers: group sizes, offsets, the contract's ranges, row indices
CID = lambda c: f"{c[0]}-{c[1]}x{c[3]}"


def sizes(bn):
    """0 first, in the middle and last; 1, BN - 1, BN, BN + 1, several tiles"""
    return [0, 1, bn - 1, 0, bn, bn + 1, 3 * bn + 8, 0]


def layout(counts, head=3, tail=5):
    off = head + np.concatenate([[0], np.cumsum(counts)])
    return off, int(off[-1]) + tail


def ranges(off, tokens):
    """the contract's [lo_g, hi_g) of include/sparsifyme.h"""
    out = []
    for g in range(len(off) - 1):
        lo = min(max(int(off[g]), 0), tokens)
        out.append((lo, min(max(int(off[g + 1]), lo), tokens)))
    return out


def indices(rng, tokens):
    """(name, x_rows, x_index)"""
    half = tokens // 2
    return [("permutation", tokens, rng.permutation(tokens)),
            ("identity", tokens, np.arange(tokens)),
            ("repeated, x_rows < tokens", half, rng.permutation(tokens) % half),
            ("x_rows > tokens", 2 * tokens + 3, rng.permutation(2 * tokens + 3)[:tokens])]


# Routings that ATTAIN the slot bound min(tokens, ceil(tokens / 64) + groups - 1) -- no block of the grid is spare -- with a real-tile
# count T = tiles_m * slots that is no multiple of 8 (the XCD remap's unit): one group; one token per group; counts = 1 mod 64.
# (counts, out of the plain case, hidden of the gated one): tiles_m = ceil(out / 64) = ceil(hidden / 32)
TIGHT = [([300], 77, 41), ([1, 1, 298], 130, 65), ([1, 1, 1, 1, 1], 77, 41), ([65, 129, 1], 130, 65), ([1], 77, 41)]
TID = lambda c: "-".join(map(str, c[0])) + f"x{c[1]}"


def tight_layout(pkg, counts, rows, inf, cus):
    off, tokens = layout(counts, head=0, tail=0)
    G = len(counts)
    assert pkg.linear24_grouped_form(tokens, G, rows, inf, cus=cus) == "tile64"
    slots = min(tokens, -(-tokens // 64) + G - 1)
    T = -(-rows // 64) * slots
    assert sum(-(-c // 64) for c in counts) == slots and T % 8 != 0, "the case must attain the bound off the remap's unit"
    return off, tokens, G
