"""Prune, check, compress, decompress and the one-pass prune + compress, per LAUNCH CLASS, on padded and guarded operands (-m gpu).

Every logical m x k operand lies at an element offset inside a larger buffer, with ld >= k and an optional gap in the batch stride.
Everything in an INPUT outside the logical regions is the type's quiet NaN (a padding element that enters a selection wins it);
everything in an OUTPUT outside what the call may write is the sentinel 0x5A5A / 0x5A5A5A5A: padding columns, gaps, GUARD elements
before the base and at least GUARD after the last logical element.  The blob has exactly sm_compress24_size bytes with a guard behind
it; d_valid sits between guard words.  After each call every sentinel keeps its bits and an out-of-place input is bit-identical.

Each case FIRST asserts, through the sm_*_form queries on the device, that the call takes the class its row names (the same tables
are pinned without a GPU, one-pass rows at 256 CUs, by test_prune_cases.py): a case that reaches another kernel fails, never skips.

The reference is never the library: the oracle's prune24 / prune24_check / compress24 / decompress24 on compact copies and, for the
STRIP rule, the numpy restatement np_strip_prune.  Every comparison is bit for bit; this file holds no tolerance.

launch classes (include/sparsifyme.h, sm_*_form):
  prune STRIP / check   strip_scalar, strip_vec, strip_flat_scalar, strip_flat_vec
  prune TILE            tile2, span (16-bit only), element_vec, element_scalar
  compress              flat, rowspan (16-bit only), general_vec, general_scalar
  decompress            vec, scalar
  one-pass              onepass_tile, onepass_tile_noblob (16-bit only), onepass_strip -- each FLAT or per batch, lpr_log2 3 .. 6, nj 1 or more,
                        grid capped or not; fallback_tall_span (16-bit only), fallback_tall, fallback_per_batch; not_supported
"""
from collections import namedtuple

import numpy as np
import pytest

from guard_testlib import ByteRegion, Guarded, dev_bits as dev, seed

pytestmark = pytest.mark.gpu

TILE, STRIP = 0, 1
GUARD = 64                      # elements before every base and (at least) behind every last logical element
TYPES = ("f16", "bf16", "f32")
ELT = {"f16": 2, "bf16": 2, "f32": 4}
FAM = {"f16": "16", "bf16": "16", "f32": "32"}
NP = {"f16": np.uint16, "bf16": np.uint16, "f32": np.uint32}
QNAN = {"f16": 0x7E00, "bf16": 0x7FC0, "f32": 0x7FC00000}
SENT = {"f16": 0x5A5A, "bf16": 0x5A5A, "f32": 0x5A5A5A5A}
SIGN = {"f16": 0x8000, "bf16": 0x8000, "f32": 0x80000000}
# 14 patterns per type: +-0, +-smallest subnormal, largest subnormal, smallest normal, +-1, largest finite, +-inf, three NaNs (quiet,
# sign set and all ones, signalling)
POOL = {
    "f16": [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x3C00, 0xBC00, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0xFFFF, 0x7C01],
    "bf16": [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x3F80, 0xBF80, 0x7F7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFFF, 0x7F81],
    "f32": [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0x7F800000,
            0xFF800000, 0x7FC00000, 0xFFFFFFFF, 0x7F800001],
}


# ---------------------------------------------------------------------------------------------
# number formats, the numpy restatement of STRIP
# ---------------------------------------------------------------------------------------------
def rand_bits(rng, n, ty, ties=False):
    """Finite random values as bit patterns (ties: small integers, many equal magnitudes)."""
    x = rng.integers(-3, 4, n).astype(np.float32) if ties else rng.standard_normal(n).astype(np.float32)
    if ty == "f16":
        return x.astype(np.float16).view(np.uint16).copy()
    if ty == "bf16":
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x.view(np.uint32).copy()


def pool_strips(ty):
    """All 14^4 = 38 416 strips of the pool, strip after strip (153 664 elements)."""
    p = np.array(POOL[ty], dtype=NP[ty])
    g = np.stack(np.meshgrid(p, p, p, p, indexing="ij"), axis=-1)
    return g.reshape(-1).copy()


def np_strip_prune(bits, m, k, ty):
    """STRIP restated: keys are the bits with the sign cleared; the two largest keys of every 1 x 4 strip are kept, ties go to the lower
    index; pruned positions become +0.  A row's last, partial strip is completed with zeros.  bits: compact m x k."""
    k4 = (k + 3) // 4 * 4
    a = np.zeros((m, k4), dtype=NP[ty])
    a[:, :k] = bits.reshape(m, k)
    s = a.reshape(-1, 4)
    key = (s & ~np.array(SIGN[ty], dtype=NP[ty])).astype(np.int64)
    rank = np.zeros(s.shape, dtype=np.int64)
    for i in range(4):
        for j in range(4):
            if i != j:
                rank[:, i] += (key[:, j] > key[:, i]) | ((key[:, j] == key[:, i]) & (j < i))
    out = np.where(rank < 2, s, 0).astype(NP[ty]).reshape(m, k4)
    return out[:, :k].reshape(-1).copy()


def np_strip_nnz_gt2(bits, m, k, ty):
    """Per strip: more than two elements whose key is not zero (what the check flags)."""
    k4 = (k + 3) // 4 * 4
    a = np.zeros((m, k4), dtype=NP[ty])
    a[:, :k] = bits.reshape(m, k)
    key = a.reshape(-1, 4) & ~np.array(SIGN[ty], dtype=NP[ty])
    return (key != 0).sum(axis=1) > 2


def orc_prune(orc, bits, m, k, alg, ty, batch=1):
    """The oracle on a compact copy; TILE per batch matrix (a tile never straddles two matrices)."""
    if alg == STRIP or batch == 1 or m % 4 == 0:
        return orc.prune24(bits, m * batch, k, k, alg, bf16=ty == "bf16")
    return np.concatenate([orc.prune24(np.ascontiguousarray(bits[b * m * k:(b + 1) * m * k]), m, k, k, alg, bf16=ty == "bf16") for b in range(batch)])


# ---------------------------------------------------------------------------------------------
# padded, guarded buffers
# ---------------------------------------------------------------------------------------------
class Pad(Guarded):
    """`batch` logical m x k matrices inside a buffer: base = GUARD + off elements, ld = k + ld_pad, stride = m * ld + gap.  fill: "nan"
    (an input) or "sent" (an output).  The buffer ends GUARD elements behind the last logical one, so a read or a write of a whole last row
    of ld leaves it.  extra: more elements behind that (the one-pass operands: see Blob)."""

    def __init__(self, ty, m, k, ld_pad=0, batch=1, gap=0, off=0, fill="nan", data=None, extra=0):
        self.ty, self.m, self.k, self.batch = ty, m, k, batch
        self.ld, base = k + ld_pad, GUARD + off
        self.stride = m * self.ld + gap
        self.fill = QNAN[ty] if fill == "nan" else SENT[ty]
        n = base + (batch - 1) * self.stride + (m - 1) * self.ld + k + GUARD + extra
        idx = (base + np.arange(batch)[:, None, None] * self.stride + np.arange(m)[None, :, None] * self.ld + np.arange(k)[None, None, :]).reshape(-1)
        Guarded.__init__(self, n, self.fill, NP[ty], base, idx)
        self.h = self.host
        assert self.idx[-1] + 1 + GUARD + extra == n
        if data is not None:
            self.h[self.idx] = data
        self.d = self.p = None

    def addr(self, origin):
        """The operand's address when the buffer starts at `origin` (a 16-byte multiple): what a query is asked with, without a device."""
        return origin + self.base * ELT[self.ty]

    def to_dev(self):
        import torch
        self.d = self.to_device().dev.view({"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[self.ty])
        self.p = self.d[self.base:]
        return self

    def logical(self, arr=None):
        return (self.read() if arr is None else arr)[self.idx]

    def matrix(self, b):
        """Device view of batch matrix b (the pointer a per-matrix call gets)."""
        return self.d[self.base + b * self.stride:]

    def assert_outside_kept(self, what):
        Guarded.assert_outside_kept(self, lambda n, first: f"{what}: {n} elements outside the logical operand changed, first at element "
                                                           f"{first - self.base} from the base")

    def assert_unchanged(self, what):
        assert self.unchanged(), f"{what}: the buffer changed"


class Blob(ByteRegion):
    """Exactly sm_compress24_size bytes at a 16-byte aligned address, sentinel bytes before and behind.  back: the guard behind it in blob
    sizes -- 8 where a wave of the one-pass kernel walks several (g, j) units of a row with nj > 1 (at most 7 row groups in ONEPASS_CASES):
    a mis-stepped counter then writes a stage plane that lies in the guard, where it is seen, not beyond it.  This guard and the `extra`
    2 k elements behind the one-pass operands (Pad) are what keeps the seeded mutation 5 of profiles/mutation_prune_classes.txt, and any
    real defect of that kind, inside the test's own allocations."""
    OUTSIDE, WRITTEN = "bytes outside the blob's reported size were written", "the blob was written"

    def __init__(self, gpu, m, k, ty, batch, back=1):
        self.size = gpu.compress24_size(m, k, ELT[ty], batch)
        self.front = 256
        self.back = max(256, back * ((self.size + 255) // 256 * 256))
        ByteRegion.__init__(self, self.size, self.front, self.back, 16)
        self.d = self.dev

    def result(self, what):
        return self.check(what)

    def assert_untouched(self, what):
        self.check(what, untouched=True)


class Flag:
    """d_valid between guard words."""
    START = 0x5A5A5A5A

    def __init__(self):
        import torch
        self.d = torch.full((9,), self.START, dtype=torch.int32, device="cuda")
        self.p = self.d[4:]

    def value(self, what):
        import torch
        torch.cuda.synchronize()
        g = self.d.cpu().numpy()
        assert (g[:4] == self.START).all() and (g[5:] == self.START).all(), f"{what}: a word next to d_valid was written"
        return int(g[4])


def seed_of(*xs):
    return seed(0x2404, *xs)


# ---------------------------------------------------------------------------------------------
# the case tables (shared with test_prune_cases.py, which pins every row without a GPU)
# ---------------------------------------------------------------------------------------------
# off_*: ELEMENTS the base is moved by (16-bit: 1, 2, 4, 8 elements = 2, 4, 8, 16 bytes; fp32: 1, 2, 4 = 4, 8, 16 bytes)
PruneCase = namedtuple("PruneCase", "name fam alg m k ld_pad off_in off_out cls span_rows", defaults=(0,))
PRUNE_CASES = [
    # ---- STRIP, 16-bit: vec = both bases 16-byte aligned and ld % 8 == 0; flat = ld == k and k % 8 == 0
    PruneCase("strip flat vec", "16", STRIP, 37, 72, 0, 0, 0, "strip_flat_vec"),
    PruneCase("strip flat vec, base +16 B", "16", STRIP, 37, 72, 0, 8, 8, "strip_flat_vec"),
    PruneCase("strip flat scalar, base +2 B", "16", STRIP, 37, 72, 0, 1, 1, "strip_flat_scalar"),
    PruneCase("strip flat scalar, out +8 B", "16", STRIP, 37, 72, 0, 0, 4, "strip_flat_scalar"),
    PruneCase("strip vec, ragged k", "16", STRIP, 37, 75, 5, 0, 0, "strip_vec"),
    PruneCase("strip scalar by ld", "16", STRIP, 37, 75, 2, 0, 0, "strip_scalar"),
    PruneCase("strip scalar by ld == k odd", "16", STRIP, 37, 75, 0, 0, 0, "strip_scalar"),
    PruneCase("strip scalar, base +2 B", "16", STRIP, 37, 75, 5, 1, 1, "strip_scalar"),
    PruneCase("strip scalar, base +4 B", "16", STRIP, 37, 75, 5, 2, 2, "strip_scalar"),
    PruneCase("strip scalar, in +8 B", "16", STRIP, 37, 75, 5, 4, 0, "strip_scalar"),
    PruneCase("strip scalar by ld and base", "16", STRIP, 37, 75, 2, 1, 1, "strip_scalar"),
    # ---- TILE, 16-bit
    PruneCase("tile2, m % 4 != 0", "16", TILE, 38, 72, 0, 0, 0, "tile2"),
    PruneCase("tile2, ld > k, base +16 B", "16", TILE, 38, 72, 8, 8, 8, "tile2"),
    PruneCase("span, several spans, short last span off 16 B", "16", TILE, 50, 147, 0, 0, 0, "span", 24),
    PruneCase("span, m < 8", "16", TILE, 5, 147, 0, 0, 0, "span", 24),
    PruneCase("span, k % 4 == 2, m % 4 != 0", "16", TILE, 131, 30, 0, 0, 0, "span", 64),
    PruneCase("span, k = 4095", "16", TILE, 9, 4095, 0, 0, 0, "span", 8),
    PruneCase("span, base +16 B", "16", TILE, 50, 147, 0, 8, 8, "span", 24),
    PruneCase("element scalar, k = 4097 contiguous", "16", TILE, 9, 4097, 0, 0, 0, "element_scalar"),
    PruneCase("element vec, contiguous ragged k = 4100", "16", TILE, 9, 4100, 0, 0, 0, "element_vec"),
    PruneCase("element vec by ld % 8", "16", TILE, 38, 72, 4, 0, 0, "element_vec"),
    PruneCase("element vec by k % 8, ld > k", "16", TILE, 38, 76, 4, 0, 0, "element_vec"),
    PruneCase("element vec, base +8 B", "16", TILE, 38, 72, 0, 4, 4, "element_vec"),
    PruneCase("element vec, span shape with base +8 B", "16", TILE, 38, 76, 0, 4, 4, "element_vec"),
    PruneCase("element scalar by ld", "16", TILE, 38, 75, 2, 0, 0, "element_scalar"),
    PruneCase("element scalar, base +2 B", "16", TILE, 38, 72, 0, 1, 1, "element_scalar"),
    PruneCase("element scalar, base +4 B", "16", TILE, 38, 72, 0, 2, 2, "element_scalar"),
    PruneCase("element scalar, out +2 B only", "16", TILE, 38, 72, 0, 0, 1, "element_scalar"),
    PruneCase("element scalar by ld and base", "16", TILE, 38, 75, 2, 1, 1, "element_scalar"),
    # ---- STRIP, fp32: vec = 16-byte aligned and ld % 4 == 0
    PruneCase("strip flat vec", "32", STRIP, 37, 72, 0, 0, 0, "strip_flat_vec"),
    PruneCase("strip flat scalar, base +4 B", "32", STRIP, 37, 72, 0, 1, 1, "strip_flat_scalar"),
    PruneCase("strip flat scalar, base +8 B", "32", STRIP, 37, 72, 0, 2, 2, "strip_flat_scalar"),
    PruneCase("strip flat vec, base +16 B", "32", STRIP, 37, 72, 0, 4, 4, "strip_flat_vec"),
    PruneCase("strip vec, ragged k", "32", STRIP, 37, 75, 1, 0, 0, "strip_vec"),
    PruneCase("strip scalar by ld", "32", STRIP, 37, 75, 2, 0, 0, "strip_scalar"),
    PruneCase("strip scalar, base +4 B", "32", STRIP, 37, 75, 1, 1, 1, "strip_scalar"),
    PruneCase("strip scalar by ld and base", "32", STRIP, 37, 75, 2, 2, 2, "strip_scalar"),
    # ---- TILE, fp32
    PruneCase("element vec", "32", TILE, 38, 72, 0, 0, 0, "element_vec"),
    PruneCase("element vec, ragged k, ld > k, base +16 B", "32", TILE, 38, 75, 1, 4, 4, "element_vec"),
    PruneCase("element scalar by ld", "32", TILE, 38, 75, 2, 0, 0, "element_scalar"),
    PruneCase("element scalar, base +4 B", "32", TILE, 38, 72, 0, 1, 1, "element_scalar"),
    PruneCase("element scalar, base +8 B", "32", TILE, 38, 72, 0, 2, 2, "element_scalar"),
    PruneCase("element scalar by ld and base", "32", TILE, 38, 75, 2, 1, 1, "element_scalar"),
    PruneCase("element scalar, k = 147 contiguous", "32", TILE, 50, 147, 0, 0, 0, "element_scalar"),
]

CompressCase = namedtuple("CompressCase", "name fam m k ld_pad batch gap off cls dcls")     # dcls: the class of decompress on this layout
COMPRESS_CASES = [
    CompressCase("flat", "16", 37, 128, 0, 2, 0, 0, "flat", "vec"),
    CompressCase("flat, base +16 B", "16", 37, 64, 0, 1, 0, 8, "flat", "vec"),
    CompressCase("rowspan, ld == k = 147, M % 32 != 0, partial last chunk", "16", 45, 147, 0, 1, 0, 0, "rowspan", "scalar"),
    CompressCase("rowspan, ld > k, two batches", "16", 20, 147, 5, 2, 0, 0, "rowspan", "vec"),
    CompressCase("rowspan, k % 64 == 0 with ld > k", "16", 37, 128, 8, 2, 0, 0, "rowspan", "vec"),
    CompressCase("rowspan, ld = 767", "16", 5, 147, 620, 1, 0, 0, "rowspan", "scalar"),
    CompressCase("general vec by ld = 768", "16", 5, 147, 621, 1, 0, 0, "general_vec", "vec"),
    CompressCase("general vec by a stride gap", "16", 37, 128, 0, 2, 8, 0, "general_vec", "vec"),
    CompressCase("general scalar by a stride gap of one", "16", 37, 128, 0, 2, 1, 0, "general_scalar", "scalar"),
    CompressCase("general scalar, base +2 B", "16", 37, 128, 0, 2, 0, 1, "general_scalar", "scalar"),
    CompressCase("general scalar, base +8 B, ragged k", "16", 45, 147, 0, 1, 0, 4, "general_scalar", "scalar"),
    CompressCase("flat", "32", 37, 128, 0, 2, 0, 0, "flat", "vec"),
    CompressCase("general vec, ragged k, ld > k", "32", 45, 147, 1, 2, 0, 0, "general_vec", "vec"),
    CompressCase("general vec by k % 64", "32", 37, 72, 0, 2, 0, 0, "general_vec", "vec"),
    CompressCase("general vec by a stride gap", "32", 37, 128, 0, 2, 4, 0, "general_vec", "vec"),
    CompressCase("general scalar by ld", "32", 45, 147, 0, 2, 0, 0, "general_scalar", "scalar"),
    CompressCase("general scalar by a stride gap of one", "32", 37, 128, 0, 2, 1, 0, "general_scalar", "scalar"),
    CompressCase("general scalar, base +4 B", "32", 37, 128, 0, 2, 0, 1, "general_scalar", "scalar"),
    CompressCase("general scalar, base +8 B", "32", 37, 128, 0, 1, 0, 2, "general_scalar", "scalar"),
]

# the one-pass kernel and the fallback.  form: with A_out, blob and flag all given, out of place; TILE without a blob is onepass_tile_noblob
# for the 16-bit types (variant "no_blob").  flat / lpr / nj: the plan; None for the fallback.
OnePassCase = namedtuple("OnePassCase", "name fam alg m k ld_pad batch gap off form flat lpr nj")
ONEPASS_CASES = [
    OnePassCase("tile flat k=64", "any", TILE, 36, 64, 0, 2, 0, 0, "onepass_tile", True, 3, 1),
    OnePassCase("tile per batch (m % 4) k=128", "any", TILE, 38, 128, 0, 2, 0, 0, "onepass_tile", False, 4, 1),
    OnePassCase("tile per batch (gap, ld > k) k=256", "any", TILE, 36, 256, 8, 2, 16, 8, "onepass_tile", False, 5, 1),
    OnePassCase("tile flat k=512", "any", TILE, 37, 512, 0, 1, 0, 0, "onepass_tile", True, 6, 1),
    OnePassCase("tile flat k=192 nj=3", "any", TILE, 200, 192, 0, 1, 0, 0, "onepass_tile", True, 3, 3),
    OnePassCase("tile per batch k=1152 nj=9", "any", TILE, 50, 1152, 0, 2, 0, 0, "onepass_tile", False, 4, 9),
    OnePassCase("strip flat k=128", "any", STRIP, 36, 128, 0, 2, 0, 0, "onepass_strip", True, 4, 1),
    OnePassCase("strip per batch (m % 4) k=64", "any", STRIP, 38, 64, 0, 2, 0, 0, "onepass_strip", False, 3, 1),
    OnePassCase("strip per batch k=192 nj=3", "any", STRIP, 101, 192, 8, 2, 0, 0, "onepass_strip", False, 3, 3),
    OnePassCase("strip flat k=1152 nj=9", "any", STRIP, 100, 1152, 0, 1, 0, 0, "onepass_strip", True, 4, 9),
    OnePassCase("strip flat k=256", "any", STRIP, 37, 256, 0, 1, 0, 0, "onepass_strip", True, 5, 1),
    OnePassCase("strip per batch (gap) k=512", "any", STRIP, 36, 512, 0, 2, 8, 0, "onepass_strip", False, 6, 1),
    # ---- the three launches
    OnePassCase("fallback tall + span with the flag", "16", TILE, 20, 147, 0, 2, 0, 0, "fallback_tall_span", None, None, None),
    OnePassCase("fallback tall, no span (ld > k)", "16", TILE, 20, 147, 5, 2, 0, 0, "fallback_tall", None, None, None),
    OnePassCase("fallback tall, STRIP with m % 4 != 0", "any", STRIP, 21, 147, 0, 2, 0, 0, "fallback_tall", None, None, None),
    OnePassCase("fallback tall, fp32 TILE", "32", TILE, 20, 147, 0, 2, 0, 0, "fallback_tall", None, None, None),
    OnePassCase("fallback tall by a moved base, k % 64 == 0", "any", TILE, 36, 64, 0, 2, 0, 1, "fallback_tall", None, None, None),
    OnePassCase("fallback per batch, odd matrices 2 B (fp32: 4 B) aligned", "any", TILE, 21, 147, 0, 3, 0, 0, "fallback_per_batch", None, None, None),
    OnePassCase("fallback per batch, odd matrices 8 B aligned", "16", TILE, 21, 76, 0, 3, 0, 0, "fallback_per_batch", None, None, None),
    OnePassCase("fallback per batch, odd matrices 8 B aligned", "32", TILE, 21, 74, 0, 3, 0, 0, "fallback_per_batch", None, None, None),
    OnePassCase("fallback per batch by a gap, STRIP", "any", STRIP, 20, 147, 0, 2, 3, 0, "fallback_per_batch", None, None, None),
]
VARIANTS = ("out_of_place", "in_place", "no_out", "no_blob", "no_flag")
# the per-batch fallback calls sm_prune24_* once per matrix, at b * strideA: the class each of those calls reaches, by (case name, family).
# 21 x 147 16-bit: matrices 6174 bytes apart (2- and 4-byte aligned); 21 x 76: 3192 bytes apart (8, then 16); fp32 rows of 147 and 74
# elements are no 16-byte multiples, so their class does not come from the base
PER_MATRIX = {
    ("fallback per batch, odd matrices 2 B (fp32: 4 B) aligned", "16"): ("span", "element_scalar", "element_scalar"),
    ("fallback per batch, odd matrices 2 B (fp32: 4 B) aligned", "32"): ("element_scalar", "element_scalar", "element_scalar"),
    ("fallback per batch, odd matrices 8 B aligned", "16"): ("span", "element_vec", "span"),
    ("fallback per batch, odd matrices 8 B aligned", "32"): ("element_scalar", "element_scalar", "element_scalar"),
    ("fallback per batch by a gap, STRIP", "16"): ("strip_scalar", "strip_scalar"),
    ("fallback per batch by a gap, STRIP", "32"): ("strip_scalar", "strip_scalar"),
}


def fams(cases):
    """(case, type) for every type of the case's family."""
    return [(c, ty) for c in cases for ty in TYPES if c.fam in ("any", FAM[ty])]


def cid(ct):
    return "%s-%s" % (ct[0].name.replace(" ", "_"), ct[1])


def capped_rows(cus):
    """The smallest row count at k = 512 (lpr_log2 = 6: one tile row per wave unit, four per workgroup) whose grid exceeds 8 x cus."""
    return 128 * cus + 1


def onepass_expect(c, ty, variant):
    """The form the variant of a one-pass case must reach."""
    if variant == "no_blob" and c.form == "onepass_tile" and ELT[ty] == 2:
        return "onepass_tile_noblob"
    if variant == "no_out" and c.form.startswith("fallback"):
        # nothing is pruned, so the span form is not asked; TILE + blob without A_out is refused off the one-pass kernel
        return "not_supported" if c.alg == TILE else c.form
    return c.form


def query_prune(pkg, c, ty, a_in, a_out):
    return pkg.prune24_form(a_in, a_out, c.m, c.k, c.k + c.ld_pad, ELT[ty], c.alg, with_span_rows=True)


def query_compress(pkg, c, ty, a, blob):
    ld = c.k + c.ld_pad
    return pkg.compress24_form(a, blob, c.m, c.k, ld, c.batch, c.m * ld + c.gap, ELT[ty])


def query_decompress(pkg, c, ty, blob, a):
    ld = c.k + c.ld_pad
    return pkg.decompress24_form(blob, a, c.m, c.k, ld, c.batch, c.m * ld + c.gap, ELT[ty])


def query_onepass(pkg, c, ty, a_in, a_out, blob, cus=0):
    ld = c.k + c.ld_pad
    return pkg.prune24_compress24_form(a_in, a_out, c.m, c.k, ld, c.batch, c.m * ld + c.gap, blob, ELT[ty], c.alg, cus=cus)


# ---------------------------------------------------------------------------------------------
# prune and check
# ---------------------------------------------------------------------------------------------
def run_prune(gpu, orc, ty, alg, m, k, ld_pad, off_in, off_out, data, cls, span_rows=0, what=""):
    """Out of place into a sentinel buffer, then in place; both against `want` = the oracle on the compact copy.  Returns want."""
    src = Pad(ty, m, k, ld_pad, off=off_in, data=data).to_dev()
    dst = Pad(ty, m, k, ld_pad, off=off_out, fill="sent").to_dev()
    got_cls = gpu.prune24_form(src.p, dst.p, m, k, src.ld, ELT[ty], alg, with_span_rows=True)
    assert got_cls == (cls, span_rows), f"{what}: the call reaches {got_cls}, not {(cls, span_rows)}"
    want = orc_prune(orc, data, m, k, alg, ty)
    gpu.prune24(src.p, dst.p, m, k, src.ld, alg)
    dst.assert_outside_kept(what + " out of place")
    src.assert_unchanged(what + " out of place: the input")
    got = dst.logical()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what} out of place: {bad.size} elements differ from the oracle, first at (row, col) {np.unravel_index(bad[:4], (m, k))}"
    # in place: the input buffer's padding is NaN and must stay NaN
    inp = Pad(ty, m, k, ld_pad, off=off_out, data=data).to_dev()
    gpu.prune24(inp.p, inp.p, m, k, inp.ld, alg)
    inp.assert_outside_kept(what + " in place")
    assert np.array_equal(inp.logical(), want), f"{what} in place differs from the oracle"
    return want


@pytest.mark.parametrize("ct", fams(PRUNE_CASES), ids=cid)
def test_prune_class(gpu, orc, ct):
    c, ty = ct
    rng = np.random.default_rng(seed_of("prune", c.name, ty))
    for ties in (False, True):
        data = rand_bits(rng, c.m * c.k, ty, ties)
        want = run_prune(gpu, orc, ty, c.alg, c.m, c.k, c.ld_pad, c.off_in, c.off_out, data, c.cls, c.span_rows, f"{c.name} {ty} ties={ties}")
        if c.alg == STRIP:
            assert np.array_equal(want, np_strip_prune(data, c.m, c.k, ty)), "the numpy restatement of STRIP differs from the oracle"


# the check reads one operand: the STRIP rows whose class does not come from the other base
CHECK_CASES = [c for c in PRUNE_CASES if c.alg == STRIP and c.off_in == c.off_out]


@pytest.mark.parametrize("ct", fams(CHECK_CASES), ids=cid)
def test_check_class(gpu, orc, ct):
    """The check on the oracle's pruned matrix inside NaN padding returns 0; with ONE strip made dense -- the first strip, the last strip of
    the last row, the partial tail item of a middle row when k % 8 != 0 -- it returns 1."""
    c, ty = ct
    m, k = c.m, c.k
    rng = np.random.default_rng(seed_of("check", c.name, ty))
    pruned = orc_prune(orc, rand_bits(rng, m * k, ty), m, k, STRIP, ty)
    one = np.array(POOL[ty][6], dtype=NP[ty])
    spots = [(0, 0), (m - 1, (k - 1) // 4 * 4)] + ([(m // 2, k // 8 * 8)] if k % 8 else [])
    flag = Flag()
    for spot in [None] + spots:
        data = pruned.copy().reshape(m, k)
        if spot is not None:
            r, c0 = spot
            if k - c0 < 3:           # a last strip of one or two columns cannot hold three values: the strip before it
                c0 -= 4
            data[r, c0:c0 + 4] = one
        data = data.reshape(-1)
        src = Pad(ty, m, k, c.ld_pad, off=c.off_in, data=data).to_dev()
        assert gpu.prune24_check_form(src.p, flag.p, m, k, src.ld, ELT[ty]) == c.cls, f"{c.name}: the check reaches another class"
        gpu.prune24_check(src.p, m, k, src.ld, flag.p)
        want = orc.prune24_check(data, m, k, k)
        assert want == (0 if spot is None else 1)
        assert flag.value(c.name) == want, f"{c.name} {ty}: check with a dense strip at {spot} returns {flag.value(c.name)}, the oracle {want}"
        src.assert_unchanged(c.name + ": the check's input")


# ---------------------------------------------------------------------------------------------
# compress and decompress
# ---------------------------------------------------------------------------------------------
def run_compress(gpu, orc, ty, c, data, what):
    src = Pad(ty, c.m, c.k, c.ld_pad, c.batch, c.gap, c.off, data=data).to_dev()
    blob = Blob(gpu, c.m, c.k, ty, c.batch)
    got_cls = gpu.compress24_form(src.p, blob.p, c.m, c.k, src.ld, c.batch, src.stride, ELT[ty])
    assert got_cls == c.cls, f"{what}: the call reaches {got_cls}, not {c.cls}"
    gpu.compress24(src.p, c.m, c.k, src.ld, c.batch, src.stride, blob.p)
    got = blob.result(what)
    src.assert_unchanged(what + ": the input")
    want = orc.compress24(data, c.m, c.k, c.k, c.batch)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} blob bytes differ from the oracle, first at {bad[:8]} of {want.size}"
    return want


@pytest.mark.parametrize("ct", fams(COMPRESS_CASES), ids=cid)
def test_compress_class(gpu, orc, ct):
    c, ty = ct
    rng = np.random.default_rng(seed_of("compress", c.name, ty))
    data = rand_bits(rng, c.batch * c.m * c.k, ty)
    run_compress(gpu, orc, ty, c, data, f"{c.name} {ty} unpruned")
    run_compress(gpu, orc, ty, c, orc_prune(orc, data, c.m, c.k, TILE, ty, c.batch), f"{c.name} {ty} TILE-pruned")
    run_compress(gpu, orc, ty, c, orc_prune(orc, rand_bits(rng, data.size, ty, True), c.m, c.k, STRIP, ty, c.batch), f"{c.name} {ty} STRIP-pruned ties")


@pytest.mark.parametrize("ct", fams(COMPRESS_CASES), ids=cid)
def test_decompress_class(gpu, orc, ct):
    """The oracle's blob into a sentinel-filled padded A: the m x k regions equal the oracle's decompress, the padding survives."""
    import torch
    c, ty = ct
    rng = np.random.default_rng(seed_of("decompress", c.name, ty))
    data = rand_bits(rng, c.batch * c.m * c.k, ty)
    ob = orc.compress24(data, c.m, c.k, c.k, c.batch)
    want = orc.decompress24(ob, c.m, c.k, c.k, NP[ty], c.batch)
    assert np.array_equal(want, np_strip_prune(data, c.batch * c.m, c.k, ty))
    dst = Pad(ty, c.m, c.k, c.ld_pad, c.batch, c.gap, c.off, fill="sent").to_dev()
    dblob = torch.from_numpy(ob).cuda()
    got_cls = gpu.decompress24_form(dblob, dst.p, c.m, c.k, dst.ld, c.batch, dst.stride, ELT[ty])
    assert got_cls == c.dcls, f"{c.name}: decompress reaches {got_cls}, not {c.dcls}"
    gpu.decompress24(dblob, c.m, c.k, dst.ld, c.batch, dst.stride, dst.p)
    dst.assert_outside_kept(c.name + " decompress")
    assert np.array_equal(dst.logical(), want), f"{c.name} {ty}: decompress differs from the oracle"
    assert np.array_equal(dblob.cpu().numpy(), ob)


# ---------------------------------------------------------------------------------------------
# the one-pass kernel and the three-launch fallback
# ---------------------------------------------------------------------------------------------
def run_onepass(gpu, orc, ty, c, variant, data, what):
    m, k, batch, alg = c.m, c.k, c.batch, c.alg
    extra = 2 * k      # (room behind the operands for a column index that runs past its row: see Blob)
    src = Pad(ty, m, k, c.ld_pad, batch, c.gap, c.off, data=data, extra=extra).to_dev()
    if variant == "in_place":
        out = src
    elif variant == "no_out":
        out = None
    else:
        out = Pad(ty, m, k, c.ld_pad, batch, c.gap, c.off, fill="sent", extra=extra).to_dev()
    blob = None if variant == "no_blob" else Blob(gpu, m, k, ty, batch, back=8 if (c.nj or 1) > 1 else 1)
    flag = None if variant == "no_flag" else Flag()
    form, plan = gpu.prune24_compress24_form(src.p, None if out is None else out.p, m, k, src.ld, batch, src.stride, None if blob is None else blob.p, ELT[ty], alg)
    expect = onepass_expect(c, ty, variant)
    assert form == expect, f"{what}: the call reaches {form}, not {expect}"
    if form.startswith("onepass"):
        assert (plan["flat"], plan["lpr_log2"], plan["nj"], plan["capped"]) == (c.flat, c.lpr, c.nj, False), f"{what}: plan {plan}"
        if c.nj > 1:
            assert (plan["grid"] * 4) % c.nj != 0, "the wave count is a multiple of nj: the wrapped (g, j) counter is not exercised"
    if form == "fallback_per_batch" and out is not None:
        got = tuple(gpu.prune24_form(src.matrix(b), out.matrix(b), m, k, src.ld, ELT[ty], alg) for b in range(batch))
        assert got == PER_MATRIX[(c.name, FAM[ty])], f"{what}: the per-matrix prune calls reach {got}"
    args = (src.p, None if out is None else out.p, m, k, src.ld, batch, src.stride, None if blob is None else blob.p, None if flag is None else flag.p, alg)
    if form == "not_supported":
        rc = getattr(gpu.lib(), "sm_prune24_compress24_" + ty)(src.p.data_ptr(), None, m, k, src.ld, batch, src.stride, blob.p.data_ptr(),
                                                               None if flag is None else flag.p.data_ptr(), alg, None)
        assert rc == gpu.STATUS_NOT_SUPPORTED and b"TILE + blob without A_out" in gpu.lib().sm_last_error()
        blob.assert_untouched(what)
        assert flag is None or flag.value(what) == Flag.START, f"{what}: a refused call wrote the flag word"
        src.assert_unchanged(what)
        return
    gpu.prune24_compress24(*args)
    pruned = orc_prune(orc, data, m, k, alg, ty, batch)
    if out is not None:
        out.assert_outside_kept(what)
        got = out.logical()
        bad = np.flatnonzero(got != pruned)
        assert bad.size == 0, f"{what}: {bad.size} elements of A_out differ from the oracle, first at (batch, row, col) {np.unravel_index(bad[:4], (batch, m, k))}"
        # the independent check of what was written, per batch matrix
        f2 = Flag()
        for b in range(batch):
            gpu.prune24_check(out.matrix(b), m, k, out.ld, f2.p)
            assert f2.value(what) == 0, f"{what}: sm_prune24_check flags batch matrix {b} of the written A_out"
    if out is not src:
        src.assert_unchanged(what + ": the input")
    if blob is not None:
        # with A_out: compress(pruned); without (STRIP only off the one-pass kernel): the STRIP selection of A itself = the same bytes
        want = orc.compress24(pruned, m, k, k, batch)
        got = blob.result(what)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} blob bytes differ from the oracle, first at {bad[:8]} of {want.size}"
    if flag is not None:
        # without A_out the fallback derives no flag: the word is reset and stays 0
        assert flag.value(what) == 0, f"{what}: the flag is {flag.value(what)}"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ct", fams(ONEPASS_CASES), ids=cid)
def test_onepass_class(gpu, orc, ct, variant):
    c, ty = ct
    rng = np.random.default_rng(seed_of("onepass", c.name, ty))
    data = rand_bits(rng, c.batch * c.m * c.k, ty, ties=variant == "in_place")
    run_onepass(gpu, orc, ty, c, variant, data, f"{c.name} {ty} {variant}")


@pytest.mark.parametrize("ty", ["f16", "f32"])
def test_fallback_resets_a_raised_flag(gpu, orc, ty):
    """The flag word is an output: sm_prune24_check raises it on a dense batch matrix (a misaligned one), the per-batch fallback in place
    on the same buffer then leaves 0."""
    c = next(x for x in ONEPASS_CASES if x.name.startswith("fallback per batch by a gap"))
    rng = np.random.default_rng(seed_of("flag", ty))
    data = rand_bits(rng, c.batch * c.m * c.k, ty)
    src = Pad(ty, c.m, c.k, c.ld_pad, c.batch, c.gap, c.off, data=data).to_dev()
    flag = Flag()
    gpu.prune24_check(src.matrix(1), c.m, c.k, src.ld, flag.p)
    assert flag.value("dense") == 1 == orc.prune24_check(data, c.m * c.batch, c.k, c.k)
    assert gpu.prune24_compress24_form(src.p, src.p, c.m, c.k, src.ld, c.batch, src.stride, None, ELT[ty], STRIP)[0] == "fallback_per_batch"
    gpu.prune24_compress24(src.p, src.p, c.m, c.k, src.ld, c.batch, src.stride, None, flag.p, STRIP)
    assert flag.value("pruned") == 0
    src.assert_outside_kept("fallback in place")


# rows beyond the capped grid's first round of units (k = 512: a unit is one tile row, a round 128 rows per CU).  "smallest": the one tile
# row that caps the grid -- only the first wave takes a second unit, the one-row m % 4 tail; "many waves": 129 tile rows more, so 129
# waves stride, the last of them on to a 3-row tail; "third unit": a second whole round and those 129, so every wave takes a second unit
# and 129 a third
CAPPED_ROUNDS = {"smallest": (1, 0), "many waves": (1, 514), "third unit": (2, 514)}     # name -> (whole rounds, rows beyond them + 1)


@pytest.mark.parametrize("size", list(CAPPED_ROUNDS))
@pytest.mark.parametrize("alg", [TILE, STRIP], ids=["tile", "strip"])
@pytest.mark.parametrize("ty", ["f16", "f32"])
def test_onepass_capped_grid(gpu, orc, ty, alg, size):
    """The grid capped at 8 workgroups per CU, at k = 512: the smallest row count whose grid exceeds the cap (m % 4 == 1), and the row
    counts of CAPPED_ROUNDS at which many waves stride on to a second and a third unit.  STRIP against the oracle on the whole operand;
    TILE against the oracle on row bands -- the first 64 rows, a band around every row where the first wave's next unit begins, a band
    around the row where the last striding wave's last unit begins, the last band with its m % 4 tail -- and bit for bit over the whole
    operand against sm_prune24 + sm_compress24 on the same input.  sm_prune24_check on the written A_out returns 0."""
    import torch
    k = 512
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rounds, beyond = CAPPED_ROUNDS[size]
    m = capped_rows(cus) + (rounds - 1) * 128 * cus + beyond
    assert capped_rows(cus) == 128 * cus + 1 and m * k < 80e6
    form, plan = gpu.prune24_compress24_form(0x1000, 0x2000, m, k, k, 1, m * k, 0x3000, ELT[ty], alg)
    assert form == ("onepass_tile" if alg == TILE else "onepass_strip") and plan["capped"] and plan["grid"] == 8 * cus and plan["flat"], (form, plan)
    _, below = gpu.prune24_compress24_form(0x1000, 0x2000, capped_rows(cus) - 1, k, k, 1, m * k, 0x3000, ELT[ty], alg)
    assert not below["capped"] and below["grid"] == 8 * cus
    rng = np.random.default_rng(seed_of("capped", ty, alg))
    data = rand_bits(rng, m * k, ty)
    src = Pad(ty, m, k, data=data).to_dev()
    out = Pad(ty, m, k, fill="sent").to_dev()
    blob, flag = Blob(gpu, m, k, ty, 1), Flag()
    assert gpu.prune24_compress24_form(src.p, out.p, m, k, k, 1, m * k, blob.p, ELT[ty], alg)[1]["capped"]
    gpu.prune24_compress24(src.p, out.p, m, k, k, 1, m * k, blob.p, flag.p, alg)
    out.assert_outside_kept("capped")
    got, gblob = out.logical(), blob.result("capped")
    assert flag.value("capped") == 0
    f2 = Flag()
    gpu.prune24_check(out.p, m, k, k, f2.p)
    assert f2.value("capped") == 0, "sm_prune24_check flags the written A_out"
    if alg == STRIP:
        want = orc.prune24(data, m, k, k, STRIP)
        assert np.array_equal(got, want), "A_out differs from the oracle"
        assert np.array_equal(want, np_strip_prune(data, m, k, ty))
        assert np.array_equal(gblob, orc.compress24(want, m, k, k, 1)), "the blob differs from the oracle"
        return
    nwaves = plan["grid"] * 4            # lpr_log2 = 6, nj = 1: unit u of the launch is tile row u; wave 0 takes units 0, nwaves, 2 nwaves ...
    units = (m + 3) // 4
    starts = [0] + [4 * u for u in range(nwaves, units, nwaves)] + [(m - 1) // 4 * 4]
    assert (units - 1) // nwaves == rounds and (units - 1) % nwaves == beyond // 4      # the last wave to take a unit in the last round
    assert len(starts) == rounds + 2 and starts[1] == 4 * nwaves and starts[rounds] == 4 * rounds * nwaves
    for r in sorted(set(starts)):
        lo, hi = max(0, r - 32) // 4 * 4, min(m, r + 32)
        band = np.ascontiguousarray(data[lo * k:hi * k])
        want = orc.prune24(band, hi - lo, k, k, TILE, bf16=False)
        assert np.array_equal(got[lo * k:hi * k], want), f"A_out differs from the oracle in rows {lo} .. {hi}"
    # the staged pair on the same input, whole operand
    a2, b2 = Pad(ty, m, k, data=data).to_dev(), Blob(gpu, m, k, ty, 1)
    gpu.prune24(a2.p, a2.p, m, k, k, TILE)
    gpu.compress24(a2.p, m, k, k, 1, m * k, b2.p)
    assert np.array_equal(a2.logical(), got), "A_out differs from sm_prune24"
    assert np.array_equal(b2.result("staged"), gblob), "the blob differs from sm_prune24 + sm_compress24"


# ---------------------------------------------------------------------------------------------
# adversarial values through every form of each rule
# ---------------------------------------------------------------------------------------------
POOL_M, POOL_K = 2401, 64            # 38 416 strips = 2401 rows of 16 strips
StripForm = namedtuple("StripForm", "name fam op m k ld_pad off cls batch gap", defaults=(1, 0))
STRIP_FORMS = [
    StripForm("prune flat vec", "any", "prune", POOL_M, POOL_K, 0, 0, "strip_flat_vec"),
    StripForm("prune flat scalar", "any", "prune", POOL_M, POOL_K, 0, 1, "strip_flat_scalar"),
    StripForm("prune vec", "any", "prune", POOL_M, POOL_K, 8, 0, "strip_vec"),
    StripForm("prune scalar", "any", "prune", POOL_M, POOL_K, 8, 1, "strip_scalar"),
    StripForm("compress flat", "any", "compress", POOL_M, POOL_K, 0, 0, "flat"),
    StripForm("compress rowspan", "16", "compress", 5488, 28, 0, 0, "rowspan"),
    StripForm("compress rowspan ld > k", "16", "compress", POOL_M, POOL_K, 8, 0, "rowspan"),
    StripForm("compress general vec", "32", "compress", POOL_M, POOL_K, 8, 0, "general_vec"),
    StripForm("compress general vec by ld = 768", "16", "compress", POOL_M, POOL_K, 704, 0, "general_vec"),
    StripForm("compress general vec, 7 batches with a gap", "any", "compress", 343, POOL_K, 0, 0, "general_vec", 7, 8),
    StripForm("compress general scalar", "any", "compress", POOL_M, POOL_K, 0, 1, "general_scalar"),
    StripForm("compress general scalar ragged", "any", "compress", 5488, 28, 1, 1, "general_scalar"),
    StripForm("one-pass strip", "any", "onepass", POOL_M, POOL_K, 0, 0, "onepass_strip"),
    StripForm("one-pass strip ld > k", "any", "onepass", POOL_M, POOL_K, 8, 0, "onepass_strip"),
    StripForm("one-pass strip per batch (m % 4, gap)", "any", "onepass", 343, POOL_K, 0, 0, "onepass_strip", 7, 8),
]


@pytest.fixture(scope="module")
def pool_refs(orc):
    """Per type: the pool's strips, the oracle's STRIP prune of them and its blobs for the shapes of STRIP_FORMS (computed once, never
    changed)."""
    refs = {}
    for ty in TYPES:
        data = pool_strips(ty)
        pruned = orc.prune24(data, POOL_M, POOL_K, POOL_K, STRIP, bf16=ty == "bf16")
        assert np.array_equal(pruned, np_strip_prune(data, POOL_M, POOL_K, ty)), "the numpy restatement of STRIP differs from the oracle on the pool"
        shapes = sorted({(f.m, f.k, f.batch) for f in STRIP_FORMS if f.op != "prune"})
        refs[ty] = dict(data=data, pruned=pruned, blob={(m, k, b): orc.compress24(data, m, k, k, b) for m, k, b in shapes})
        for v in [data, pruned] + list(refs[ty]["blob"].values()):
            v.setflags(write=False)
    return refs


@pytest.mark.parametrize("ct", fams(STRIP_FORMS), ids=cid)
def test_strip_rule_on_the_pool(gpu, orc, pool_refs, ct):
    """All 14^4 strips of the specials pool through one STRIP form, against the oracle (and, through pool_refs, the numpy restatement)."""
    f, ty = ct
    ref = pool_refs[ty]
    data, m, k = ref["data"], f.m, f.k
    what = f"{f.name} {ty}"
    dst = None
    if f.op == "prune":
        src = Pad(ty, m, k, f.ld_pad, off=f.off, data=data).to_dev()
        dst = Pad(ty, m, k, f.ld_pad, off=f.off, fill="sent").to_dev()
        assert gpu.prune24_form(src.p, dst.p, m, k, src.ld, ELT[ty], STRIP) == f.cls
        gpu.prune24(src.p, dst.p, m, k, src.ld, STRIP)
        dst.assert_outside_kept(what)
        got, want = dst.logical(), ref["pruned"]
    elif f.op == "compress":
        src = Pad(ty, m, k, f.ld_pad, f.batch, f.gap, f.off, data=data).to_dev()
        blob = Blob(gpu, m, k, ty, f.batch)
        assert gpu.compress24_form(src.p, blob.p, m, k, src.ld, f.batch, src.stride, ELT[ty]) == f.cls
        gpu.compress24(src.p, m, k, src.ld, f.batch, src.stride, blob.p)
        got, want = blob.result(what), ref["blob"][(m, k, f.batch)]
    else:
        src = Pad(ty, m, k, f.ld_pad, f.batch, f.gap, f.off, data=data, extra=2 * k).to_dev()
        dst = Pad(ty, m, k, f.ld_pad, f.batch, f.gap, f.off, fill="sent", extra=2 * k).to_dev()
        blob, flag = Blob(gpu, m, k, ty, f.batch), Flag()
        form, plan = gpu.prune24_compress24_form(src.p, dst.p, m, k, src.ld, f.batch, src.stride, blob.p, ELT[ty], STRIP)
        assert form == f.cls and plan["flat"] == (f.batch == 1), (form, plan)
        gpu.prune24_compress24(src.p, dst.p, m, k, src.ld, f.batch, src.stride, blob.p, flag.p, STRIP)
        dst.assert_outside_kept(what)
        assert flag.value(what) == 0
        assert np.array_equal(dst.logical(), ref["pruned"]), f"{what}: A_out differs from the oracle"
        got, want = blob.result(what), ref["blob"][(m, k, f.batch)]
    src.assert_unchanged(what)
    if dst is not None:     # the independent check of what was written, per batch matrix
        f2 = Flag()
        for b in range(f.batch):
            gpu.prune24_check(dst.matrix(b), m, k, dst.ld, f2.p)
            assert f2.value(what) == 0, f"{what}: sm_prune24_check flags batch matrix {b} of the written output"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} differences from the oracle, first at {bad[:8]}"


CHECK_LAYOUTS = {"strip_flat_vec": (0, 0), "strip_flat_scalar": (0, 1), "strip_vec": (8, 0), "strip_scalar": (3, 1)}     # class -> (ld_pad, off)


@pytest.mark.parametrize("layout", list(CHECK_LAYOUTS))
@pytest.mark.parametrize("ty", TYPES)
def test_check_on_the_pool(gpu, orc, pool_refs, ty, layout):
    """The check on the pool: every strip, 1; the pruned strips, 0; the strips with at most two non-zero keys alone, 0; and single strips
    [v v v 0] and [v v -0 +0] for every pool value v, each with the oracle's verdict (NaN and subnormals count, -0 does not)."""
    ref = pool_refs[ty]
    ld_pad, off = CHECK_LAYOUTS[layout]
    flag = Flag()

    def check(data, m, k, want_cls=None):
        src = Pad(ty, m, k, ld_pad, off=off, data=data).to_dev()
        if want_cls:
            assert gpu.prune24_check_form(src.p, flag.p, m, k, src.ld, ELT[ty]) == want_cls
        gpu.prune24_check(src.p, m, k, src.ld, flag.p)
        v = flag.value("pool")
        assert v == orc.prune24_check(np.ascontiguousarray(data), m, k, k), f"check of {m} x {k} differs from the oracle"
        return v

    assert check(ref["data"], POOL_M, POOL_K, layout) == 1
    assert check(ref["pruned"], POOL_M, POOL_K, layout) == 0
    dense = np_strip_nnz_gt2(ref["data"], POOL_M, POOL_K, ty)
    sparse = ref["data"].reshape(-1, 4)[~dense]
    assert sparse.shape[0] % 2 == 0 and sparse.shape[0] > 1000
    assert check(sparse.reshape(-1).copy(), sparse.shape[0] // 2, 8) == 0
    zero, nzero = POOL[ty][0], POOL[ty][1]
    for v in POOL[ty]:
        nonzero = (v & ~SIGN[ty]) != 0
        assert check(np.array([v, v, v, zero], dtype=NP[ty]), 1, 4) == (1 if nonzero else 0), hex(v)
        assert check(np.array([v, v, nzero, zero], dtype=NP[ty]), 1, 4) == 0, hex(v)


TILE_M, TILE_K = 64, 128
TileForm = namedtuple("TileForm", "name fam op k ld_pad off cls")
TILE_FORMS = [
    TileForm("tile2", "16", "prune", 128, 0, 0, "tile2"),
    TileForm("span", "16", "prune", 132, 0, 0, "span"),
    TileForm("element vec", "16", "prune", 128, 0, 4, "element_vec"),
    TileForm("element scalar", "16", "prune", 128, 0, 1, "element_scalar"),
    TileForm("element vec", "32", "prune", 128, 0, 0, "element_vec"),
    TileForm("element scalar", "32", "prune", 128, 0, 1, "element_scalar"),
    TileForm("one-pass tile", "any", "onepass", 128, 0, 0, "onepass_tile"),
    TileForm("one-pass tile no blob", "16", "onepass_noblob", 128, 8, 0, "onepass_tile_noblob"),
]


def tile_data(ty, k):
    """TILE_M x k: 4 x 4 tiles drawn from the pool (upper half of the rows) and from small integers, for ties (lower half)."""
    rng = np.random.default_rng(seed_of("tiles", ty, k))
    pool = np.array(POOL[ty], dtype=NP[ty])
    top = pool[rng.integers(0, len(pool), (TILE_M // 2) * k)]
    # every other pool tile is thinned with zeros so that finite sums decide as well
    top = np.where(rng.random(top.size) < 0.3, np.array(POOL[ty][int(rng.integers(0, 2))], dtype=NP[ty]), top).astype(NP[ty])
    return np.concatenate([top, rand_bits(rng, (TILE_M // 2) * k, ty, ties=True)])


@pytest.mark.parametrize("ct", fams(TILE_FORMS), ids=cid)
def test_tile_rule_on_adversarial_tiles(gpu, orc, ct):
    f, ty = ct
    m, k = TILE_M, f.k
    data = tile_data(ty, k)
    want = orc.prune24(data, m, k, k, TILE, bf16=ty == "bf16")
    what = f"{f.name} {ty}"
    src = Pad(ty, m, k, f.ld_pad, off=f.off, data=data, extra=2 * k).to_dev()
    dst = Pad(ty, m, k, f.ld_pad, off=f.off, fill="sent", extra=2 * k).to_dev()
    if f.op == "prune":
        assert gpu.prune24_form(src.p, dst.p, m, k, src.ld, ELT[ty], TILE) == f.cls
        gpu.prune24(src.p, dst.p, m, k, src.ld, TILE)
    else:
        blob = Blob(gpu, m, k, ty, 1) if f.op == "onepass" else None
        flag = Flag()
        assert gpu.prune24_compress24_form(src.p, dst.p, m, k, src.ld, 1, src.stride, None if blob is None else blob.p, ELT[ty], TILE)[0] == f.cls
        gpu.prune24_compress24(src.p, dst.p, m, k, src.ld, 1, src.stride, None if blob is None else blob.p, flag.p, TILE)
        assert flag.value(what) == 0
        if blob is not None:
            assert np.array_equal(blob.result(what), orc.compress24(want, m, k, k, 1)), f"{what}: the blob differs from the oracle"
    dst.assert_outside_kept(what)
    src.assert_unchanged(what)
    got = dst.logical()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} elements differ from the oracle, first at (row, col) {np.unravel_index(bad[:4], (m, k))}"
    f2 = Flag()
    gpu.prune24_check(dst.p, m, k, dst.ld, f2.p)
    assert f2.value(what) == 0, f"{what}: sm_prune24_check flags the written A_out"


# ---------------------------------------------------------------------------------------------
# refusals: the documented status, nothing written
# ---------------------------------------------------------------------------------------------
INVALID, NOT_SUPPORTED = 1, 2
# name -> (entry, overrides of the call, status, text of sm_last_error)
REFUSALS = {
    "prune null A_in": ("prune", dict(a_in=None), INVALID, b"sm_prune24: invalid argument"),
    "prune null A_out": ("prune", dict(a_out=None), INVALID, b"sm_prune24: invalid argument"),
    "prune ld < k": ("prune", dict(ld=-1), INVALID, b"sm_prune24: invalid argument"),
    "prune bad alg": ("prune", dict(alg=2), INVALID, b"sm_prune24: invalid argument"),
    "check null A": ("check", dict(a_in=None), INVALID, b"sm_prune24_check: invalid argument"),
    "check null d_valid": ("check", dict(flag=None), INVALID, b"sm_prune24_check: invalid argument"),
    "check ld < k": ("check", dict(ld=-1), INVALID, b"sm_prune24_check: invalid argument"),
    "compress null A": ("compress", dict(a_in=None), INVALID, b"sm_compress24: invalid argument"),
    "compress null blob": ("compress", dict(blob=None), INVALID, b"sm_compress24: invalid argument"),
    "compress ld < k": ("compress", dict(ld=-1), INVALID, b"sm_compress24: invalid argument"),
    "compress misaligned blob": ("compress", dict(blob_off=8), INVALID, b"blob must be 16-byte aligned"),
    "decompress null A": ("decompress", dict(a_out=None), INVALID, b"sm_decompress24: invalid argument"),
    "decompress null blob": ("decompress", dict(blob=None), INVALID, b"sm_decompress24: invalid argument"),
    "decompress ld < k": ("decompress", dict(ld=-1), INVALID, b"sm_decompress24: invalid argument"),
    "onepass null A_in": ("onepass", dict(a_in=None), INVALID, b"sm_prune24_compress24_%s: invalid argument"),
    "onepass ld < k": ("onepass", dict(ld=-1), INVALID, b"sm_prune24_compress24_%s: invalid argument"),
    "onepass bad alg": ("onepass", dict(alg=-1), INVALID, b"sm_prune24_compress24_%s: invalid argument"),
    "onepass misaligned blob": ("onepass", dict(blob_off=4), INVALID, b"sm_prune24_compress24_%s: invalid argument"),
    "onepass TILE + blob without A_out, ragged k": ("onepass", dict(a_out=None, alg=TILE), NOT_SUPPORTED, b"TILE + blob without A_out"),
    "onepass TILE + blob without A_out, moved base": ("onepass", dict(a_out=None, alg=TILE, k=64, in_off=2), NOT_SUPPORTED, b"TILE + blob without A_out"),
}
REFUSAL_M, REFUSAL_K = 12, 147


def refused_call(L, ty, name, a_in, a_out, blob, flag):
    """Calls the entry of REFUSALS[name] with the given addresses (ints or None) and the entry's overrides; returns (status, message)."""
    entry, over, status, text = REFUSALS[name]
    m, k = REFUSAL_M, over.get("k", REFUSAL_K)
    ld = k + over.get("ld", 0)
    alg = over.get("alg", STRIP)
    a_in = None if "a_in" in over else a_in + over.get("in_off", 0)
    a_out = None if "a_out" in over else a_out
    blob = None if "blob" in over else blob + over.get("blob_off", 0)
    flag = None if "flag" in over else flag
    sfx = ty
    if entry == "prune":
        rc = getattr(L, "sm_prune24_" + sfx)(a_in, a_out, m, k, ld, alg, None)
    elif entry == "check":
        rc = getattr(L, "sm_prune24_check_" + sfx)(a_in, m, k, ld, flag, None)
    elif entry == "compress":
        rc = getattr(L, "sm_compress24_" + sfx)(a_in, m, k, ld, 1, m * ld, blob, None)
    elif entry == "decompress":
        rc = getattr(L, "sm_decompress24_" + sfx)(blob, m, k, ld, 1, m * ld, a_out, None)
    else:
        rc = getattr(L, "sm_prune24_compress24_" + sfx)(a_in, a_out, m, k, ld, 1, m * ld, blob, flag, alg, None)
    return rc, L.sm_last_error()


def refusal_text(name, ty):
    text = REFUSALS[name][3]
    return text % ty.encode() if b"%s" in text else text


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_leaves_everything_untouched(gpu, ty, name):
    rng = np.random.default_rng(seed_of("refusal", name, ty))
    data = rand_bits(rng, REFUSAL_M * REFUSAL_K, ty)
    src = Pad(ty, REFUSAL_M, REFUSAL_K, data=data).to_dev()
    out = Pad(ty, REFUSAL_M, REFUSAL_K, fill="sent").to_dev()
    blob, flag = Blob(gpu, REFUSAL_M, REFUSAL_K, ty, 1), Flag()
    rc, msg = refused_call(gpu.lib(), ty, name, src.p.data_ptr(), out.p.data_ptr(), blob.p.data_ptr(), flag.p.data_ptr())
    assert rc == REFUSALS[name][2] and refusal_text(name, ty) in msg, (rc, msg)
    src.assert_unchanged(name)
    out.assert_unchanged(name)
    blob.assert_untouched(name)
    assert flag.value(name) == Flag.START, f"{name}: the refused call wrote the flag word"


# ---------------------------------------------------------------------------------------------
# replay: one class of each entry point captured in a hipGraph gives the eager bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
def test_graph_replay_gives_the_eager_bytes(gpu, orc, ty):
    import torch
    m, k, batch = 36, 128, 2
    rng = np.random.default_rng(seed_of("replay", ty))
    data = rand_bits(rng, batch * m * k, ty)
    src = Pad(ty, m, k, 8, batch, 16, 8, data=data, extra=2 * k).to_dev()

    def outputs():
        return dict(pr=Pad(ty, m, k, 8, batch, 16, 8, fill="sent", extra=2 * k).to_dev(), op=Pad(ty, m, k, 8, batch, 16, 8, fill="sent", extra=2 * k).to_dev(),
                    de=Pad(ty, m, k, 8, batch, 16, 8, fill="sent", extra=2 * k).to_dev(), b1=Blob(gpu, m, k, ty, batch), b2=Blob(gpu, m, k, ty, batch),
                    f1=Flag(), f2=Flag())

    def work(o):
        # prune (per batch matrix: the gap), check, compress, decompress, the one-pass kernel
        for b in range(batch):
            gpu.prune24(src.matrix(b), o["pr"].matrix(b), m, k, src.ld, TILE)
        gpu.prune24_check(o["pr"].p, m, k, src.ld, o["f1"].p)
        gpu.compress24(o["pr"].p, m, k, src.ld, batch, src.stride, o["b1"].p)
        gpu.decompress24(o["b1"].p, m, k, src.ld, batch, src.stride, o["de"].p)
        gpu.prune24_compress24(src.p, o["op"].p, m, k, src.ld, batch, src.stride, o["b2"].p, o["f2"].p, TILE)

    eager, replay = outputs(), outputs()
    assert gpu.prune24_compress24_form(src.p, eager["op"].p, m, k, src.ld, batch, src.stride, eager["b2"].p, ELT[ty], TILE)[0] == "onepass_tile"
    work(eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        work(replay)
    for o in (replay["pr"], replay["op"], replay["de"]):      # capture ran nothing
        o.d.copy_(dev(o.h, ty))
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    want = orc_prune(orc, data, m, k, TILE, ty, batch)
    for key in ("pr", "op", "de"):
        assert np.array_equal(eager[key].read(), replay[key].read()), key
        eager[key].assert_outside_kept(key)
        assert np.array_equal(eager[key].logical(), want), key
    for key in ("b1", "b2"):
        assert np.array_equal(eager[key].result(key), replay[key].result(key)), key
        assert np.array_equal(eager[key].result(key), orc.compress24(want, m, k, k, batch)), key
    for key in ("f1", "f2"):
        assert eager[key].value(key) == replay[key].value(key) == 0
