"""What the sm_rmsnorm_* tests share: the definition of include/sparsifyme.h restated in numpy -- fp32 to the operation, the sum of squares in
a stated order (sequential or pairwise; the definition leaves it open) -- the fp64 evaluation of the same definition from the same rounded
h, the bound the device is held to, the integer class on which the fp32 restatement IS the definition, and the layout builder of the GPU
test (operands at moved bases with pitches above `hidden`, NaN in the padding, guard words around every output).

16-bit values travel as uint16 bit patterns; `ty` is "f16" or "bf16"."""
import numpy as np

from guard_testlib import NAN16, f32_of, is_nan16, rne16   # noqa: F401  (the two 16-bit types as bit patterns: one set for all files; re-exported)

TYPES = ["f16", "bf16"]
MANT = {"f16": 10, "bf16": 7}                 # explicit significand bits
EMIN = {"f16": -14, "bf16": -126}             # exponent of the smallest normal
FP8 = {"e4m3": 0, "e5m2": 1}                  # SM_FP8_*


# ------------------------------------------------------------------------------------------------ the two 16-bit types
def bits_of(x, ty):
    """any real array -> the 16-bit type's bit patterns (one rounding from float32)"""
    return rne16(np.asarray(x, dtype=np.float32), ty)


def same_bits_nan_as_nan(a, b, ty):
    """bit for bit, except that a NaN equals any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (is_nan16(a, ty) & is_nan16(b, ty))))


# ------------------------------------------------------------------------------------------------ the definition
def add_round(H, D, ty):
    """h = rne16(fp32(H) + fp32(D)); without D, H unchanged"""
    if D is None:
        return np.asarray(H, dtype=np.uint16).copy()
    with np.errstate(invalid="ignore"):
        return rne16(f32_of(H, ty) + f32_of(D, ty), ty)


def sum_squares32(x, order):
    """sum over the last axis of x * x in float32: "seq" ascending j, "tree" pairwise halving"""
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (x * x).astype(np.float32)
        if order == "seq":
            return np.add.accumulate(sq, axis=-1, dtype=np.float32)[..., -1]
        n = 1
        while n < sq.shape[-1]:
            n *= 2
        sq = np.concatenate([sq, np.zeros(sq.shape[:-1] + (n - sq.shape[-1],), dtype=np.float32)], axis=-1)
        while sq.shape[-1] > 1:
            sq = (sq[..., 0::2] + sq[..., 1::2]).astype(np.float32)
        return sq[..., 0]


def norm32(h, gamma, eps, ty, order="seq"):
    """n of the definition from the rounded h (uint16 [tokens][hidden]), every operation a float32 operation; gamma uint16 [hidden] or None"""
    x = f32_of(h, ty)
    hidden = np.float32(x.shape[-1])
    with np.errstate(all="ignore"):
        ms = (sum_squares32(x, order) / hidden).astype(np.float32)
        r = (np.float32(1.0) / np.sqrt((ms + np.float32(eps)).astype(np.float32))).astype(np.float32)
        y = (x * r[..., None]).astype(np.float32)
        if gamma is not None:
            y = (y * f32_of(gamma, ty)[None, :]).astype(np.float32)
    return rne16(y, ty)


def norm64(h, gamma, eps, ty):
    """the same definition from the same rounded h in float64, not rounded to the output type"""
    x = f32_of(h, ty).astype(np.float64)
    with np.errstate(all="ignore"):
        r = 1.0 / np.sqrt((x * x).sum(axis=-1) / x.shape[-1] + float(np.float32(eps)))
        y = x * r[..., None]
        if gamma is not None:
            y = y * f32_of(gamma, ty).astype(np.float64)[None, :]
    return y


def ulp16(x, ty):
    """the spacing of the 16-bit type at |x| (float64; the subnormal spacing below the smallest normal)"""
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** EMIN[ty])))
    return 2.0 ** (np.maximum(e, EMIN[ty]) - MANT[ty])


def bound(ref, got, hidden, ty):
    """half an ulp of the output type at the larger of |ref| and |N| -- the one rounding -- plus (hidden + 8) * 2^-24 * |ref|: hidden * 2^-24
    bounds the fp32 sum of squares in any order, 8 stands for the division, the add, the square root, the division, the two multiplies
    and slack.  An allowance, not a measurement."""
    return 0.5 * ulp16(np.maximum(np.abs(ref), np.abs(got)), ty) + (hidden + 8) * 2.0 ** -24 * np.abs(ref)


def worst_ratio(n_bits, h_bits, gamma, eps, ty):
    """the worst |N - ref| / bound over the finite reference values; NaN must sit exactly where the reference has it"""
    ref = norm64(h_bits, gamma, eps, ty)
    got = f32_of(n_bits, ty).astype(np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN where the definition has none (or none where it has)"
    # a reference past the type's largest finite value may round to inf: the bound is about finite outputs
    fin &= np.isfinite(got)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float((np.abs(got - ref)[fin] / bound(ref, got, h_bits.shape[-1], ty)[fin]).max())


# ------------------------------------------------------------------------------------------------ the integer class
def integer_rows(rng, tokens, hidden, ty, special=True):
    """H, D with h = H + D integers, |h| <= 15 (|H| <= 8, |D| <= 7), gamma integers with |gamma| <= 4, as bit patterns.  special: rows with
    an inf, a NaN, both, all zeros and a single non-zero element are planted (as many as the token count allows)."""
    H = rng.integers(-8, 9, (tokens, hidden)).astype(np.float32)
    D = rng.integers(-7, 8, (tokens, hidden)).astype(np.float32)
    g = rng.integers(-4, 5, hidden).astype(np.float32)
    if special:
        plant = [("zero", None), ("inf", np.inf), ("nan", np.nan), ("ninf", -np.inf), ("both", None), ("one", None)]
        for t, (kind, val) in zip(range(tokens - 1, 0, -1), plant):       # from the last row down; row 0 stays ordinary
            j = int(rng.integers(0, hidden))
            if kind == "zero":
                H[t], D[t] = 0.0, 0.0
            elif kind == "both":
                H[t, j], D[t, (j + 1) % hidden] = np.inf, np.nan
            elif kind == "one":
                H[t], D[t] = 0.0, 0.0
                H[t, j] = 3.0
            else:
                H[t, j] = val
    return bits_of(H, ty), bits_of(D, ty), bits_of(g, ty)


def integer_class(h, gamma, ty):
    """the premise: every finite h an integer with |h| <= 15, every gamma an integer with |gamma| <= 4, and 225 * hidden < 2^24 -- every
    partial sum of S is then an exact fp32 integer in any order, so norm32 is the definition itself"""
    x = f32_of(h, ty)
    fin = np.isfinite(x)
    ok = bool(np.all(x[fin] == np.round(x[fin]))) and bool(np.all(np.abs(x[fin]) <= 15)) and 225 * x.shape[-1] < 2 ** 24
    if gamma is not None:
        gv = f32_of(gamma, ty)
        ok = ok and bool(np.all(gv == np.round(gv))) and bool(np.all(np.abs(gv) <= 4))
    return ok


# ------------------------------------------------------------------------------------------------ the layout builder (GPU test)
GUARD = 16                 # elements before (beyond the moved base) and behind every allocation
SENT16, SENT8, SENT32 = 0x2BCD, 0xA5, -12345.0


class Operand:
    """A [rows][cols] operand at a moved base inside an allocation, row pitch above cols, the rest of the allocation filled with `fill`
    (bit pattern for the 16-bit and 1-byte kinds): NaN for an input's padding, a sentinel for an output's padding and guards."""

    def __init__(self, torch, dtype, rows, cols, pitch, base, fill, dev="cuda:0"):
        self.torch, self.rows, self.cols, self.pitch, self.base = torch, rows, cols, pitch, base
        size = dtype.itemsize
        raw = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[size]
        n = base + max(rows, 1) * pitch + GUARD
        if raw is torch.float32:
            self.raw = torch.full((n,), float(fill), dtype=raw, device=dev)
        else:
            self.raw = torch.full((n,), int(np.array(fill, dtype={1: np.uint8, 2: np.uint16}[size]).view({1: np.uint8, 2: np.int16}[size])), dtype=raw, device=dev)
        self.alloc = self.raw.view(dtype)
        self.view = self.alloc.as_strided((rows, cols), (pitch, 1), base)
        self.np_dtype = {1: np.uint8, 2: np.uint16, 4: np.float32}[size]

    def load(self, bits):
        """bit patterns (or float32 for a float32 operand) into the operand's elements"""
        t = self.torch.from_numpy(np.ascontiguousarray(bits).view({1: np.uint8, 2: np.int16, 4: np.float32}[self.raw.dtype.itemsize]))
        self.raw.as_strided((self.rows, self.cols), (self.pitch, 1), self.base).copy_(t.to(self.raw.device))

    def snapshot(self):
        return self.raw.clone()

    def bits(self):
        r = self.raw.as_strided((self.rows, self.cols), (self.pitch, 1), self.base).cpu().numpy()
        return np.ascontiguousarray(r).view(self.np_dtype).copy()

    def outside_unchanged(self, before):
        """every element of the allocation that is not one of the operand's own elements still holds what `before` (a snapshot) holds"""
        a, b = self.raw.clone(), before.clone()
        for t in (a, b):
            t.as_strided((self.rows, self.cols), (self.pitch, 1), self.base).zero_()
        if a.dtype.is_floating_point:
            a, b = a.view(self.torch.int32), b.view(self.torch.int32)
        return bool((a == b).all())
