"""The implicit-GEMM convolution of csrc/conv_spmma.hip (and the im2col kernels of csrc/im2col.hip it is measured against) on GUARDED operands,
per kernel class (-m gpu).

X and B lie between quiet-NaN guards (0x7e00 / 0x7fc0, 64 elements each side; the `+x4` cases place X two halves further in: 4-byte aligned, not
16), C lies inside a larger allocation of 0x5A5A words, the workspace of the routed entry has exactly the bytes sm_conv_spmma_workspace reports,
pre-filled with 0x5A and followed by a guard.  Afterwards the guards, the inputs and the bytes around C and the workspace must hold what they
held.  With beta == 0 C starts as quiet NaN and must come out NaN-free.

The reference is NOT the library: numpy fp64 from the definition -- for each output pixel the window read straight from the NCHW X by index
arithmetic (column c * kh * kw + r * kw + u, zeros outside the image), the STRIP rule (the two largest |x| of each 1 x 4 strip, ties keep the
lower k), the product with B, alpha and beta in fp64.  Two data kinds per case: `ties` (X, B and the initial C integers in [-3, 3], (alpha, beta) in
{(1, 0), (0.5, -2)}: every partial sum is a multiple of 0.5 of magnitude <= 4.5 K + 6 < 2^24 -- asserted -- so fp32 accumulation is exact in ANY
order and ALL of C must equal the reference rounded ONCE to the output type, bit for bit, +0 and -0 equal) and `uniform` (U(-1, 1): check_close of
parity_testlib at FP16_TOL and the rounding + accumulation bound of the output type, k = the K / 2 kept terms + 2).  Every taken case also
asserts: the implicit kernel's C is bit-identical to sm_im2col_compress24 + sm_spmma for all N images; sm_im2col gives the reference's A and,
followed by sm_compress24, the same blob; sm_conv_spmma_fused_plan names the class the case is listed under.  Every declined case asserts status 2
with C untouched, and through the routed sm_conv_spmma_*: the reference with the reported workspace, status 2 without one.

Kernel classes (conv_spmma16 switches on conv_fused_rule; tests/test_conv_cases.py restates it and holds every case against it):

    class        patch DMA            condition                                     column tile: -64 for n_out <= 64, else -128
    V16          16 bytes per lane    W % 8 == 0, X 16-byte aligned, a_n <= 16      a_n: patch DMA instructions per 64-deep stage
    SMALL        4 bytes per lane     a_n <= 16                                     = ceil(nch * RI / rpi)
    LARGE        4 bytes per lane     16 < a_n <= 48
    declined     status 2             a_n > 48 (V16: > 16 falls back to 4 bytes), pitch / halves per lane > 64, kh * kw > 64, K % 64 != 0

    what the cases pin                 cases
    LARGE-128 (never launched before)  the ResNet down-sampling layer n_out 128; n_out 136 (a second tile of 8 columns); 1 x 1 on 128 channels
    partial column tiles               n_out 8, 24, 56 under the 64-column kernels, 72, 136, 200 under the 128-column ones, every family
    channel bound cbase + a_ch < Cin   Cin 16 / 48 with 2 x 2 (nch 17), Cin 4 / 12 with 4 x 4, Cin 1 / 3 with 8 x 8 (kh * kw = 64); 5 x 13: declined
    1 x 1 windows                      taken as SMALL-64 (a_n 13), as LARGE-128, at a_n 48; declined at a_n 49
    windows and borders                1 x 7, 3 x 1, pad beyond the window's reach, dilation 3 without pad (padl 6), stride 3, 7 x 7 dilation 2,
                                       OW = 2 (a tile straddles 65 output rows, RI 67)
    L at the tile edge                 L 126, 128, 140; N = 3 with L % 128 != 0
    thresholds, a case on each side    4-byte a_n 16 / 17 and 16 / 19 (SMALL / LARGE), 48 / 49 and 47 / 50 (taken / declined), V16 a_n 16 / 17
                                       (17: the 4-byte form runs it), V16 a_n 13 whose 4-byte plan needs 51, pitch / 2 = 64 (W 126) / W 128 (V16
                                       only: declined with X + 4 bytes), W 120 / 122, kh * kw 64 / 65
    special values, one per family     X with +-0, +-inf, the largest finite value and subnormals, B with +-inf: bit identity with the pair, the
                                       NaN / inf positions of the fp64 reference over the KEPT terms (0 x inf in a dropped position: no NaN)"""
import collections
import functools

import numpy as np
import pytest

from guard_testlib import (Guarded, Workspace, canon16 as canon, f64_of as bits_to_f64, is_nan16, margin_report_fixture, rne16 as f32_to_bits,
                           round_once, seed)
from parity_testlib import FP16_TOL, check_close, rand

pytestmark = pytest.mark.gpu

TYPES = ("f16", "bf16")
QNAN16 = {"f16": np.uint16(0x7E00), "bf16": np.uint16(0x7FC0)}
SENT16 = np.uint16(0x5A5A)
GUARD = 64                     # elements in front of and behind every buffer (128 bytes: the base alignment is the offset's)
INVALID, NOT_SUPPORTED = 1, 2
KINDS = ("ties", "uniform")
ABS = ((1.0, 0.0), (0.5, -2.0))
CLASSES = ("V16-64", "V16-128", "SMALL-64", "SMALL-128", "LARGE-64", "LARGE-128")
DECLINED = "declined"
FORM_NAMES = {"v16": "V16", "small4": "SMALL", "large4": "LARGE"}


def _seed(*xs):
    return seed(0x5718, *xs)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
# geom: (N, Cin, H, W, kh, kw, stride, pad, dil, n_out); cls: the class the library must report; x_off: halves X lies past a 16-byte boundary (0 or
# 2); pins: plan numbers the case is there for (held against the library's answer in tests/test_conv_cases.py and here)
ConvCase = collections.namedtuple("ConvCase", "name geom cls x_off pins", defaults=(0, None))

CONV_CASES = [
    # LARGE-128
    ConvCase("large128-resnet-down", (1, 64, 28, 28, 3, 3, 2, 1, 1, 128), "LARGE-128", 0, {"a_n": 46}),
    ConvCase("large128-n136", (2, 64, 28, 28, 3, 3, 2, 1, 1, 136), "LARGE-128", 0, {"tiles_n": 2}),
    ConvCase("large128-1x1-n136", (1, 128, 6, 6, 1, 1, 1, 0, 1, 136), "LARGE-128", 0, {"nch": 64, "a_n": 24}),
    # partial column tiles, every family
    ConvCase("small64-n8", (1, 64, 14, 14, 3, 3, 1, 1, 1, 8), "SMALL-64"),
    ConvCase("small128-n72", (1, 64, 14, 14, 3, 3, 1, 1, 1, 72), "SMALL-128"),
    ConvCase("v16-128-n200", (1, 64, 56, 56, 3, 3, 1, 1, 1, 200), "V16-128", 0, {"tiles_n": 2}),
    ConvCase("large128-n200+x4", (1, 64, 56, 56, 3, 3, 1, 1, 1, 200), "LARGE-128", 2, {"a_n": 24}),
    ConvCase("v16-64-n24-4x4", (2, 12, 16, 16, 4, 4, 2, 1, 1, 24), "V16-64"),
    ConvCase("small64-n24-4x4+x4", (2, 12, 16, 16, 4, 4, 2, 1, 1, 24), "SMALL-64", 2),
    # the channel bound
    ConvCase("cin16-2x2", (1, 16, 12, 12, 2, 2, 1, 0, 1, 64), "LARGE-64", 0, {"nch": 17}),
    ConvCase("cin48-2x2-s2", (1, 48, 12, 12, 2, 2, 2, 0, 1, 64), "LARGE-64", 0, {"nch": 17}),
    ConvCase("cin4-4x4", (1, 4, 16, 16, 4, 4, 1, 1, 1, 64), "V16-64", 0, {"nch": 5}),
    ConvCase("cin1-8x8", (1, 1, 20, 20, 8, 8, 1, 0, 1, 64), "SMALL-64", 0, {"nch": 2}),
    ConvCase("cin3-8x8-s2", (1, 3, 24, 24, 8, 8, 2, 3, 1, 64), "V16-64", 0, {"nch": 2}),
    ConvCase("khkw65", (1, 64, 18, 18, 5, 13, 1, 2, 1, 64), DECLINED),
    # 1 x 1 taken
    ConvCase("1x1-small64", (2, 64, 4, 4, 1, 1, 1, 0, 1, 64), "SMALL-64", 0, {"nch": 64, "a_n": 13}),
    # windows and borders
    ConvCase("1x7", (1, 64, 12, 16, 1, 7, 1, 3, 1, 64), "V16-64"),
    ConvCase("3x1", (1, 64, 16, 12, 3, 1, 1, 1, 1, 64), "LARGE-64"),
    ConvCase("pad3", (1, 64, 12, 12, 3, 3, 1, 3, 1, 64), "SMALL-64", 0, {"padl": 4}),
    ConvCase("dil3-nopad", (1, 64, 20, 20, 3, 3, 1, 0, 3, 64), "LARGE-64", 0, {"padl": 6}),
    ConvCase("stride3", (1, 64, 20, 20, 3, 3, 3, 1, 1, 64), "LARGE-64"),
    ConvCase("7x7-dil2", (1, 64, 20, 20, 7, 7, 1, 3, 2, 64), "LARGE-64"),
    ConvCase("ow2", (1, 64, 80, 4, 3, 3, 1, 0, 1, 64), "LARGE-64", 0, {"RI": 67}),
    # L at the tile edge
    ConvCase("L126", (1, 64, 9, 14, 3, 3, 1, 1, 1, 64), "SMALL-64"),
    ConvCase("L128", (1, 64, 8, 16, 3, 3, 1, 1, 1, 64), "V16-64"),
    ConvCase("L140", (1, 64, 10, 14, 3, 3, 1, 1, 1, 64), "SMALL-64"),
    ConvCase("L140-n3", (3, 64, 10, 14, 3, 3, 1, 1, 1, 64), "SMALL-64"),
    # SMALL / LARGE threshold
    ConvCase("a_n16-s2", (1, 64, 30, 6, 3, 3, 2, 1, 1, 64), "SMALL-64", 0, {"a_n": 16}),
    ConvCase("a_n17-s2", (1, 64, 20, 10, 3, 3, 2, 1, 1, 56), "LARGE-64", 0, {"a_n": 17}),
    ConvCase("a_n16", (2, 64, 16, 30, 3, 3, 1, 1, 1, 128), "SMALL-128", 0, {"a_n": 16}),
    ConvCase("a_n19", (2, 64, 16, 34, 3, 3, 1, 1, 1, 128), "LARGE-128", 0, {"a_n": 19}),
    # taken / declined threshold
    ConvCase("a_n48-1x1", (1, 64, 12, 6, 1, 1, 1, 0, 1, 64), "LARGE-64", 0, {"a_n": 48}),
    ConvCase("a_n49-1x1", (1, 64, 16, 4, 1, 1, 1, 0, 1, 64), DECLINED, 0, {"a_n": 49}),
    ConvCase("a_n47", (1, 64, 28, 20, 3, 3, 2, 1, 1, 72), "LARGE-128", 0, {"a_n": 47}),
    ConvCase("a_n50+x4", (1, 64, 28, 24, 3, 3, 2, 1, 1, 72), DECLINED, 2, {"a_n": 50}),      # (an aligned X: V16 takes it, next line)
    ConvCase("a_n50-v16", (1, 64, 28, 24, 3, 3, 2, 1, 1, 72), "V16-128", 0, {"a_n": 13}),
    # the limits of V16
    ConvCase("v16-a_n16", (1, 64, 4, 224, 3, 3, 1, 1, 1, 136), "V16-128", 0, {"a_n": 16}),
    ConvCase("v16-a_n17", (1, 64, 54, 8, 7, 1, 2, 0, 1, 64), "LARGE-64", 0, {"a_n": 45}),       # V16 would need 17: the 4-byte form runs it
    ConvCase("v16-a_n13", (1, 64, 32, 32, 3, 3, 2, 1, 1, 64), "V16-64", 0, {"a_n": 13}),
    ConvCase("v16-a_n13+x4", (1, 64, 32, 32, 3, 3, 2, 1, 1, 64), DECLINED, 2, {"a_n": 51}),
    # pitch
    ConvCase("w126", (1, 64, 16, 126, 3, 3, 1, 1, 1, 64), "LARGE-64", 0, {"pitch": 128}),
    ConvCase("w128", (1, 64, 16, 128, 3, 3, 1, 1, 1, 64), "V16-64", 0, {"pitch": 136}),
    ConvCase("w128+x4", (1, 64, 16, 128, 3, 3, 1, 1, 1, 64), DECLINED, 2),
    ConvCase("w120", (1, 64, 8, 120, 3, 3, 1, 1, 1, 64), "V16-64", 0, {"pitch": 128}),
    ConvCase("w122", (1, 64, 8, 122, 3, 3, 1, 1, 1, 64), "LARGE-64", 0, {"pitch": 124}),
]
# (lo, hi, plan field or None, (lo value, hi value)): the two sides of every threshold
THRESHOLDS = [("a_n16-s2", "a_n17-s2", "a_n", (16, 17)), ("a_n16", "a_n19", "a_n", (16, 19)), ("a_n48-1x1", "a_n49-1x1", "a_n", (48, 49)),
              ("a_n47", "a_n50+x4", "a_n", (47, 50)), ("v16-a_n16", "v16-a_n17", None, None), ("v16-a_n13", "v16-a_n13+x4", "a_n", (13, 51)),
              ("w126", "w128+x4", None, None), ("w128", "w128+x4", None, None), ("w120", "w122", None, None), ("cin1-8x8", "khkw65", None, None)]
SPECIAL_CASES = ("v16-64-n24-4x4", "small128-n72", "large128-1x1-n136")      # one per family, each with a partial column tile
BY_NAME = {c.name: c for c in CONV_CASES}


def out_size(size, k, s, p, d):
    return (size + 2 * p - d * (k - 1) - 1) // s + 1


def dims(geom):
    """(OH, OW, L, K)."""
    N, Cin, H, W, kh, kw, s, p, d, n_out = geom
    OH, OW = out_size(H, kh, s, p, d), out_size(W, kw, s, p, d)
    return OH, OW, OH * OW, Cin * kh * kw


def class_of(form, plan):
    return DECLINED if form == "not_taken" else f"{FORM_NAMES[form]}-{plan['bn']}"


def x_align(case):
    return 16 if case.x_off % 8 == 0 else 4 if case.x_off % 2 == 0 else 2


# ---------------------------------------------------------------------------------------------
# the reference, from the definition
# ---------------------------------------------------------------------------------------------
def window_index(geom):
    """(idx, inside), both [L][K]: where column c * kh * kw + r * kw + u of output pixel l lies in one image's [C][H][W], and whether it does."""
    N, Cin, H, W, kh, kw, s, p, d, n_out = geom
    OH, OW, L, K = dims(geom)
    ih = (np.arange(OH)[:, None] * s - p + np.arange(kh)[None, :] * d)[:, None, None, :, None]      # [OH][1][1][kh][1]
    iw = (np.arange(OW)[:, None] * s - p + np.arange(kw)[None, :] * d)[None, :, None, None, :]      # [1][OW][1][1][kw]
    c = np.arange(Cin)[None, None, :, None, None]
    shape = (OH, OW, Cin, kh, kw)
    inside = np.broadcast_to((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W), shape).reshape(L, K)
    idx = np.broadcast_to((c * H + np.clip(ih, 0, H - 1)) * W + np.clip(iw, 0, W - 1), shape).reshape(L, K)
    return idx, inside


def strip_keep(A):
    """[M][K] bool: the two largest |x| of every 1 x 4 strip, ties keep the lower k."""
    M, K = A.shape
    order = np.argsort(-np.abs(A).reshape(M, K // 4, 4), axis=-1, kind="stable")
    keep = np.zeros((M, K // 4, 4), dtype=bool)
    np.put_along_axis(keep, order[..., :2], True, axis=-1)
    return keep.reshape(M, K)


class Problem:
    """One case, data kind and type: X, B and the initial C as bits, the im2col operand and the references."""

    def __init__(self, case, kind, t):
        self.case, self.kind, self.t = case, kind, t
        N, Cin, H, W, kh, kw, s, p, d, n_out = case.geom
        OH, OW, L, K = dims(case.geom)
        self.N, self.L, self.K, self.n_out = N, L, K, n_out
        rng = np.random.default_rng(_seed("conv", case.name, kind, t if kind != "ties" else ""))
        gen = lambda n: f32_to_bits(rand(rng, n, np.float32, "ties" if kind == "ties" else "uniform"), t)
        self.X, self.B, self.C0 = gen(N * Cin * H * W), gen(K * n_out), gen(N * L * n_out)
        if kind == "special":
            self._plant_special_values(rng)
        self._refs = {}

    def _plant_special_values(self, rng):
        """X: +-0 and subnormals at a twentieth of the positions each, +-inf at a thousandth each, the largest finite value once per image (so that
        no window holds two and no fp32 partial sum overflows); B: +-1 with a few zeros and +-inf (|B| <= 1 keeps max * B finite in fp32)."""
        t, n = self.t, self.X.size // self.N
        inf, big, sub = (0x7C00, 0x7BFF, 0x03FF) if t == "f16" else (0x7F80, 0x7F7F, 0x007F)
        for val, rate in ((0x0000, 0.05), (0x8000, 0.05), (inf, 0.001), (0x8000 | inf, 0.001)):
            self.X[rng.random(self.X.size) < rate] = val
        where = rng.random(self.X.size) < 0.05
        self.X[where] = (rng.integers(1, sub + 1, int(where.sum())) | (rng.integers(0, 2, int(where.sum())) << 15)).astype(np.uint16)
        for img in range(self.N):
            self.X[img * n + rng.integers(0, n)] = big
        self.B = f32_to_bits((2 * rng.integers(0, 2, self.B.size) - 1).astype(np.float32), t)
        self.B[rng.random(self.B.size) < 0.02] = 0
        self.B[rng.random(self.B.size) < 0.002] = inf
        self.B[rng.random(self.B.size) < 0.002] = 0x8000 | inf
        assert not is_nan16(self.X, t).any() and not is_nan16(self.B, t).any()

    @functools.cached_property
    def A_bits(self):
        """[N * L][K] bits: the im2col operand, zeros outside the image."""
        idx, inside = window_index(self.case.geom)
        Ximg = self.X.reshape(self.N, -1)
        return np.concatenate([np.where(inside, Ximg[i][idx], np.uint16(0)) for i in range(self.N)])

    @functools.cached_property
    def kept(self):
        """(A in fp64 with the dropped positions zero -- finite data only --, the keep mask)."""
        A = bits_to_f64(self.A_bits, self.t)
        keep = strip_keep(A)
        return np.where(keep, A, 0.0), keep

    def reference(self, ab):
        """(ref, scale), [N * L][n_out] flattened: alpha * prune(A) B + beta * C0 (C0 unread when beta == 0) and |alpha| |prune(A)| |B| + |beta| |C0|."""
        if ab not in self._refs:
            Ak, _ = self.kept
            Bm = bits_to_f64(self.B, self.t).reshape(self.K, self.n_out)
            ref, scale = ab[0] * (Ak @ Bm), abs(ab[0]) * (np.abs(Ak) @ np.abs(Bm))
            if ab[1] != 0.0:
                c0 = bits_to_f64(self.C0, self.t).reshape(self.N * self.L, self.n_out)
                ref, scale = ref + ab[1] * c0, scale + abs(ab[1]) * np.abs(c0)
            self._refs[ab] = ((ref + 0.0).reshape(-1), scale.reshape(-1))
        return self._refs[ab]

    def reference_over_kept_terms(self):
        """alpha = 1, beta = 0 with non-finite data: the sum over the KEPT positions only (a dropped position meets no B), 32 rows at a time."""
        A = bits_to_f64(self.A_bits, self.t)
        order = np.sort(np.argsort(-np.abs(A).reshape(A.shape[0], self.K // 4, 4), axis=-1, kind="stable")[..., :2], axis=-1)
        kidx = (order + 4 * np.arange(self.K // 4)[None, :, None]).reshape(A.shape[0], self.K // 2)
        vals = np.take_along_axis(A, kidx, axis=1)
        Bm = bits_to_f64(self.B, self.t).reshape(self.K, self.n_out)
        out = np.empty((A.shape[0], self.n_out))
        with np.errstate(invalid="ignore"):
            for r0 in range(0, A.shape[0], 32):
                out[r0:r0 + 32] = (vals[r0:r0 + 32, :, None] * Bm[kidx[r0:r0 + 32]]).sum(axis=1)
        return out.reshape(-1)


@functools.lru_cache(maxsize=4)
def problem(name, kind, t):
    return Problem(BY_NAME[name], kind, t)


def assert_ties_premise(p, ref, scale):
    bound = 4.5 * p.K + 6
    assert bound < 2.0 ** 24 and scale.max() <= bound and np.array_equal(np.rint(2.0 * ref), 2.0 * ref)


# ---------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------
def Buf16(payload, guard, off=0):
    """An input (bits) between GUARD guard elements, `off` more of them in front."""
    return Guarded.around(payload, guard, GUARD + off, GUARD)


def CBuf16(payload):
    """C (bits) inside an allocation of sentinel words: GUARD in front, GUARD + 8 behind."""
    return Guarded.around(payload, SENT16, GUARD, GUARD + 8)


def c_result(C, what):
    """The logical C as bits, after asserting that every sentinel around it kept its bits."""
    size = C.idx.stop - C.idx.start
    return C.result(lambda n, first: f"{what}: {n} elements outside C were written, first at {first - GUARD} (C has {size})")


def compare(got, p, ab, what, cls):
    """All of C against the fp64 reference: `ties` bit for bit against the reference rounded once, `uniform` through check_close."""
    t = p.t
    shape = (p.N * p.L, p.n_out)
    bad = np.flatnonzero(is_nan16(got, t))
    assert bad.size == 0, f"{what}: {bad.size} NaN results (a guard read into a product, or C not written?), first at {np.unravel_index(bad[:4], shape)}"
    ref, scale = p.reference(ab)
    if p.kind == "ties":
        assert_ties_premise(p, ref, scale)
        want = round_once(ref, t)
        wrong = np.flatnonzero(canon(got) != canon(want))
        assert wrong.size == 0, (f"{what}: {wrong.size} of {got.size} results are not the once-rounded product, first at {np.unravel_index(wrong[:4], shape)}: "
                                 f"{bits_to_f64(got[wrong[:4]], t)} for {ref[wrong[:4]]}")
    else:
        check_close(bits_to_f64(got, t), ref, scale, FP16_TOL, f"conv[{cls}] {what}", p.K // 2 + 2, t)


# ---------------------------------------------------------------------------------------------
# the calls, with pointers as integers
# ---------------------------------------------------------------------------------------------
def call_fused(L, t, X, B, C, geom, ab=(1.0, 0.0)):
    return getattr(L, "sm_conv_spmma_fused_" + t)(X, B, C, *geom, ab[0], ab[1], None)


def call_routed(L, t, X, B, C, geom, ab=(1.0, 0.0), ws=None, ws_bytes=0):
    return getattr(L, "sm_conv_spmma_" + t)(X, B, C, *geom, ab[0], ab[1], ws, ws_bytes, None)


class Pair:
    """sm_im2col_compress24 + sm_spmma on the guarded X and B; the blob behind a guard of its own."""

    def __init__(self, gpu, p, dX, dB, what):
        import torch
        self.L, self.p, self.dB = gpu.lib(), p, dB
        g, t = p.case.geom, p.t
        self.nbytes = gpu.compress24_size(p.L, p.K, 2, p.N)
        self.blob = torch.full((self.nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        rc = getattr(self.L, "sm_im2col_compress24_" + t)(dX.ptr, *g[:9], self.blob.data_ptr(), None)
        assert rc == 0, f"{what}: sm_im2col_compress24 status {rc}: {self.L.sm_last_error().decode()}"
        # the two-step form: the dense A is the reference's, its blob the same bytes
        A = torch.full((p.N * p.L * p.K + GUARD,), 0x5A5A, dtype=torch.int16, device="cuda")
        rc = getattr(self.L, "sm_im2col_" + t)(dX.ptr, *g[:9], A.data_ptr(), None)
        assert rc == 0, f"{what}: sm_im2col status {rc}: {self.L.sm_last_error().decode()}"
        blob2 = torch.full_like(self.blob, 0x5A)
        rc = getattr(self.L, "sm_compress24_" + t)(A.data_ptr(), p.L, p.K, p.K, p.N, p.L * p.K, blob2.data_ptr(), None)
        assert rc == 0, f"{what}: sm_compress24 status {rc}: {self.L.sm_last_error().decode()}"
        torch.cuda.synchronize()
        a = A.cpu().numpy().view(np.uint16)
        assert np.array_equal(a[:-GUARD], p.A_bits.reshape(-1)) and (a[-GUARD:] == SENT16).all(), f"{what}: sm_im2col is not the window read by index arithmetic"
        assert torch.equal(self.blob, blob2), f"{what}: sm_im2col + sm_compress24 and sm_im2col_compress24 give different blobs"
        assert bool((self.blob[self.nbytes:] == 0x5A).all()), f"{what}: bytes behind the blob were written"

    def product(self, c0, ab):
        import torch
        p = self.p
        C = torch.from_numpy(c0.view(np.int16).copy()).cuda()
        rc = getattr(self.L, "sm_spmma_" + p.t)(self.blob.data_ptr(), self.dB.ptr, C.data_ptr(), p.L, p.n_out, p.K, p.N, 0, p.L * p.n_out, ab[0], ab[1], None)
        assert rc == 0, f"sm_spmma status {rc}: {self.L.sm_last_error().decode()}"
        torch.cuda.synchronize()
        return C.cpu().numpy().view(np.uint16)


def initial_c(p, ab):
    return p.C0 if ab[1] != 0.0 else np.full(p.C0.size, QNAN16[p.t], dtype=np.uint16)


def run_taken(gpu, case, t, kind):
    L, p = gpu.lib(), problem(case.name, kind, t)
    what0 = f"{t} {kind} {case.name} {case.geom}"
    form, plan = gpu.conv_spmma_fused_plan(*case.geom, x_align=x_align(case))
    assert class_of(form, plan) == case.cls, f"{what0}: the library reports {form} with {plan}"
    dX, dB = Buf16(p.X, QNAN16[t], off=case.x_off).to_device(), Buf16(p.B, QNAN16[t]).to_device()
    assert dX.ptr % 16 == 2 * case.x_off and dB.ptr % 16 == 0
    pair = Pair(gpu, p, dX, dB, what0)
    results = {}
    for ab in ABS:
        what = f"{what0} ab {ab}"
        c0 = initial_c(p, ab)
        C = CBuf16(c0).to_device()
        rc = call_fused(L, t, dX.ptr, dB.ptr, C.ptr, case.geom, ab)      # beta != 0: C in place
        assert rc == 0, f"{what}: status {rc}: {L.sm_last_error().decode()}"
        got = c_result(C, what)
        want = pair.product(c0, ab)
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (f"{what}: {diff.size} of {got.size} results differ from sm_im2col_compress24 + sm_spmma, first at "
                                f"{np.unravel_index(diff[:4], (p.N * p.L, p.n_out))}")
        if kind != "special":
            compare(got, p, ab, what, case.cls)
        results[ab] = got
    assert dX.unchanged() and dB.unchanged(), f"{what0}: an input or one of its guards was modified"
    return results


def run_declined(gpu, case, t, kind):
    L, p = gpu.lib(), problem(case.name, kind, t)
    what0 = f"{t} {kind} {case.name} {case.geom}"
    form, plan = gpu.conv_spmma_fused_plan(*case.geom, x_align=x_align(case))
    assert form == "not_taken", f"{what0}: the library reports {form} with {plan}"
    dX, dB = Buf16(p.X, QNAN16[t], off=case.x_off).to_device(), Buf16(p.B, QNAN16[t]).to_device()
    C = CBuf16(initial_c(p, ABS[0])).to_device()
    assert call_fused(L, t, dX.ptr, dB.ptr, C.ptr, case.geom) == NOT_SUPPORTED and C.unchanged(), f"{what0}: the implicit kernel must decline"
    assert call_routed(L, t, dX.ptr, dB.ptr, C.ptr, case.geom) == NOT_SUPPORTED and C.unchanged(), f"{what0}: without a workspace the routed entry must decline"
    need = gpu.conv_spmma_workspace(*case.geom[:9])
    assert need == gpu.compress24_size(p.L, p.K, 2, p.N) > 0
    for ab in ABS:
        what = f"{what0} routed ab {ab}"
        ws = Workspace(need)
        C = CBuf16(initial_c(p, ab)).to_device()
        rc = call_routed(L, t, dX.ptr, dB.ptr, C.ptr, case.geom, ab, ws.ptr, need)
        assert rc == 0, f"{what}: status {rc}: {L.sm_last_error().decode()}"
        got = c_result(C, what)
        ws.check(what)
        compare(got, p, ab, what, "routed")
    assert dX.unchanged() and dB.unchanged(), f"{what0}: an input or one of its guards was modified"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.name)
def test_conv_on_guarded_operands(gpu, case, t):
    for kind in KINDS:
        (run_declined if case.cls == DECLINED else run_taken)(gpu, case, t, kind)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", SPECIAL_CASES)
def test_conv_special_values(gpu, name, t):
    """+-0, +-inf, the largest finite value and subnormals in X, +-inf in B: the implicit kernel equals the pair bit for bit (run_taken), and C has the
    NaN and inf positions of the fp64 sum over the kept terms -- a dropped position next to an inf in B gives no NaN."""
    case = BY_NAME[name]
    got = run_taken(gpu, case, t, "special")[ABS[0]]       # alpha = 1, beta = 0
    p = problem(name, "special", t)
    ref = p.reference_over_kept_terms()
    g = bits_to_f64(got, t)
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any(), "the case does not reach every kind of result"
    assert np.array_equal(np.isnan(g), np.isnan(ref)), f"{name} {t}: NaN where the sum over the kept terms has none, or the reverse"
    inf = np.isinf(ref)
    assert np.array_equal(g[inf], ref[inf]), f"{name} {t}: the infinities differ"
    # a dense product of the zero-filled operand WOULD have NaN there: the check above is not vacuous
    Ak, keep = p.kept
    Bm = bits_to_f64(p.B, t).reshape(p.K, p.n_out)
    dropped_meets_inf = ((~keep).astype(np.float64) @ np.isinf(Bm).astype(np.float64)).reshape(-1) > 0
    assert (dropped_meets_inf & ~np.isnan(ref)).any()


# ---------------------------------------------------------------------------------------------
# refusals: decided before any device work (tests/test_conv_cases.py runs the same table without a device)
# ---------------------------------------------------------------------------------------------
_GOOD = (1, 64, 8, 8, 3, 3, 1, 1, 1, 64)
# name -> (geom, bytes added to X, bytes added to B, status)
REFUSALS = {
    "X at + 2 bytes": (_GOOD, 2, 0, NOT_SUPPORTED),
    "n_out % 8 != 0": (_GOOD[:9] + (68,), 0, 0, NOT_SUPPORTED),
    "B at + 2 bytes": (_GOOD, 0, 2, NOT_SUPPORTED),
    "odd W": ((1, 64, 8, 9, 3, 3, 1, 1, 1, 64), 0, 0, NOT_SUPPORTED),
    "zero stride": ((1, 64, 8, 8, 3, 3, 0, 1, 1, 64), 0, 0, INVALID),
    "zero dilation": ((1, 64, 8, 8, 3, 3, 1, 1, 0, 64), 0, 0, INVALID),
    "window larger than the padded input": ((1, 64, 4, 4, 5, 5, 1, 0, 1, 64), 0, 0, INVALID),
}


def call_refusal(L, name, t, X, B, C, routed=False):
    geom, xo, bo, _ = REFUSALS[name]
    return call_routed(L, t, X + xo, B + bo, C, geom) if routed else call_fused(L, t, X + xo, B + bo, C, geom)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_conv_refusals(gpu, name):
    import torch
    x = torch.zeros(8192, dtype=torch.float16, device="cuda")
    L = gpu.lib()
    for t in TYPES:
        for routed in (False, True):
            rc = call_refusal(L, name, t, x.data_ptr(), x.data_ptr(), x.data_ptr(), routed)
            assert rc == REFUSALS[name][3], f"{name} {t} routed={routed}: status {rc}: {L.sm_last_error().decode()}"
    assert not bool(x.any())


# ---------------------------------------------------------------------------------------------
# margins of this file's `uniform` comparisons, appended to the session's report: the worst per class, then the worst cases
# ---------------------------------------------------------------------------------------------
_conv_margin_report = margin_report_fixture(
    "{n} comparisons of tests/test_gpu_conv.py against the numpy fp64 convolution; err / bound (check_close), worst per class:", per_first_word=True)
