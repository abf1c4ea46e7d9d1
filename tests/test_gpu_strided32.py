"""The fp32 dense, 2:4 and bf16-split matmuls on PADDED operands, per launch class (-m gpu).

Every case places the logical operands in larger buffers with a guard region at both ends (base offsets, lda > k, gaps in the batch
strides).  A and B outside the logical operand hold a quiet fp32 NaN, C outside the logical result holds 0x5A5A5A5A: a kernel that reads
padding into a product shows a NaN, one that writes outside its tile changes a sentinel; A and B must come back bit for bit.  The
references are NOT the library: the gathered logical A (for the 2:4 entry points pruned by the oracle's STRIP rule on the compact copy)
times the gathered B in numpy fp64, alpha and beta applied in fp64.  Two data kinds per case: `ties` (integers in [-3, 3], k <= 256,
(alpha, beta) in {(1, 0), (0.5, -2)}: every product, partial sum, bf16 piece and scale is exact, so C must equal the fp64 result
converted to fp32 bit for bit -- the premise is asserted per case) and `uniform` (U(-1, 1): check_close at FP32_TOL, the fmaf-chain
kernels also at 1e-5, the split forms under parity_testlib.split_bound).  Stated contracts (include/sparsifyme.h), bit for bit with the
right-hand side on compact copies: sm_spmma_fused_f32 == sm_gemm_rowmajor_f32 of the oracle-pruned A; sm_spmma_fused_f32_split_prepared
== sm_spmma_fused_f32_split (B overwritten with NaN between prepare and the product).

Launch classes (csrc/gemm_f32.hip, csrc/spmma_f32_split.hip) and the cases that pin them; m = 200 unless said, batch 2 (`tall`: 3):

    class (CLASS_NEEDS key)        dispatch                        cases
    dma<64,64>                     gemm_f32.hip:609, 866           m = 40, n = 40, per-batch layouts only (a fold gives M = 80 > 64)
    dma<64,128>                    gemm_f32.hip:609, 866           m = 40; n = 72 and 200, per-batch layouts
    dma<128,64>                    gemm_f32.hip:610, 871           n = 40 and 104, every layout (fused: P24 = 2, the register selection)
    dma<128,128>                   gemm_f32.hip:610, 871           n = 136 (ragged second column tile; fused: P24 = 1, in LDS)
    generic<64,64>                 gemm_f32.hip:605, 615           dense only: k = 72, n = 37, lda+1, sA+2, a_off1, b_off1, k = 5
    generic<128,64>                gemm_f32.hip:615                dense only, sized from the CU count: test_dense_generic_128x64_tiles
    staged dma<64,4,1>             gemm_f32.hip:933-936            k in {64, 192}, n in {40, 104}
    staged generic                 gemm_f32.hip:938 (dispatch32<1>) k = 72, n = 37, m = 201, b_off1, sB+2
    split<64>                      spmma_f32_split.hip:826-830     n = 40
    split<128> ant                 spmma_f32_split.hip:729, 826    n = 104 (tiles_n == 1)
    split cols                     spmma_f32_split.hip:821         n = 136 (second half ragged against 128) and 256
    split<128> nt                  spmma_f32_split.hip:733, 826    n = 264 (three column tiles, the last 8 wide)
    span<64>, span<128>            spmma_f32_split.hip:767, 805    k in {72, 147}, n = 40 / 104 (k = 147, n = 104 exceeds the LDS: REFUSALS), batch 3 tall, compact and off16
    thresholds, same operands      M <= 64, N <= 64, N <= 128 (dma); n <= 64, 128, 256 (split): test_both_sides_of_each_threshold
    folded tall grid               gemm_f32.hip:832, 861, 927; spmma_f32_split.hip:801: compact, lda+4, lda+16, off16, c_off1, tall, ab
    per-batch grid (b > 0)         sA+64, sB+16, sB=kn, sC+8, sC+3, all; the fold must not fire on a gap: sentinels of the gap (result())
    vector store on batch 0, per-element on batch 1: sC+3;  per-element everywhere: c_off1, n = 37
    refusals                       REFUSALS (also called without a device by test_strided32_cases.py)"""
import collections
import ctypes

import numpy as np
import pytest

from guard_testlib import Guarded, Layout, Strided, margin_report_fixture, seed
from parity_testlib import FP32_TOL, MARGINS, bits, check_close, rand, split_bound

pytestmark = pytest.mark.gpu

QNAN = np.uint32(0x7FC00000)
SENT = np.uint32(0x5A5A5A5A)
GUARD = 64                     # floats in front of and behind every buffer (a multiple of 4: the base alignment is the offset's)
INVALID, NOT_SUPPORTED = 1, 2
KINDS = ("ties", "uniform")
AB = (0.5, -2.0)


# ---------------------------------------------------------------------------------------------
# the layout builder
# ---------------------------------------------------------------------------------------------
def _seed(*xs):
    return seed(0x5718, *xs)


LAYOUTS = {
    "compact": dict(),
    "lda+4": dict(lda_pad=4),
    "lda+16": dict(lda_pad=16),
    "lda+1": dict(lda_pad=1),                    # the row alignment is lost
    "sA+64": dict(gapA=64),                      # breaks the fold: the per-batch grid runs
    "sA+2": dict(gapA=2),
    "sB+16": dict(gapB=16),                      # a B per batch, with a gap
    "sB=kn": dict(gapB=0),                       # packed, per batch
    "sB+2": dict(gapB=2),
    "sC+8": dict(gapC=8),
    "sC+3": dict(gapC=3),                        # batch 1's C leaves the vector-store alignment, batch 0 keeps it
    "off16": dict(offA=4, offB=8, offC=12),
    "c_off1": dict(offC=1),
    "a_off1": dict(offA=1),
    "b_off1": dict(offB=1),
    "tall": dict(batch=3),                       # contiguous: one tall matrix, a row tile straddles two batches
    "tall+off16": dict(batch=3, offA=4, offB=8, offC=12),
    "ab": dict(alpha=AB[0], beta=AB[1]),
    "all": dict(lda_pad=16, gapA=64, gapB=16, gapC=8, offA=4, offB=8, offC=12, alpha=AB[0], beta=AB[1]),
}


def layout_of(fam, lname):
    """The layout of a matmul case: the split forms take a per-batch B only packed, so their `all` has strideB = k * n."""
    d = dict(LAYOUTS[lname])
    if fam == "split" and lname == "all":
        d["gapB"] = 0
    return Layout(**d)


def draw(rng, kind, batch, nb, m, n, k):
    return (rand(rng, batch * m * k, np.float32, kind).reshape(batch, m, k), rand(rng, nb * k * n, np.float32, kind).reshape(nb, k, n),
            rand(rng, batch * m * n, np.float32, kind).reshape(batch, m, n))


class Problem(Strided):
    """Padded host buffers (uint32 bit patterns), index maps of the logical operands, the references and -- after to_device() -- the
    device copies.  kind: "ties" or "uniform"; data: (A [batch][m][k], B [nb][k][n], C0 [batch][m][n]) instead of a draw from rng."""

    def __init__(self, m, n, k, lay, kind, rng=None, data=None):
        Strided.__init__(self, m, n, k, lay, GUARD + lay.offA, GUARD + lay.offB, GUARD + lay.offC)
        self.kind = kind
        batch, nb = self.batch, self.nb
        self.gA = Guarded(self.baseA + (batch - 1) * self.sA + m * self.lda + GUARD, QNAN, np.uint32, self.baseA, self.iA)
        self.gB = Guarded(self.baseB + (nb - 1) * self.sBe + k * n + GUARD, QNAN, np.uint32, self.baseB, self.iB)
        self.gC = Guarded(self.baseC + (batch - 1) * self.sC + m * n + GUARD, SENT, np.uint32, self.baseC, self.iC)
        self.A, self.B, self.C = self.gA.host, self.gB.host, self.gC.host
        a, b, c0 = draw(rng, kind, batch, nb, m, n, k) if data is None else data
        assert a.shape == (batch, m, k) and b.shape == (nb, k, n) and c0.shape == (batch, m, n)
        self.A[self.iA] = bits(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1)
        self.B[self.iB] = bits(np.ascontiguousarray(b, dtype=np.float32)).reshape(-1)
        self.reads_c = lay.beta != 0.0
        self.C0 = bits(np.ascontiguousarray(c0, dtype=np.float32)).reshape(-1) if self.reads_c else np.full(batch * m * n, SENT, dtype=np.uint32)
        self.C[self.iC] = self.C0
        self.outC = self.gC.outside
        self._refs = {}

    def a_compact(self):
        return np.ascontiguousarray(self.A[self.iA])

    def b_compact(self):
        return np.ascontiguousarray(self.B[self.iB])

    # ---- references (numpy fp64; the oracle only prunes) ---------------------------------------
    def pruned_bits(self, orc):
        return orc.prune24(self.a_compact(), self.batch * self.m, self.k, self.k, orc.STRIP)

    def reference(self, orc, pruned):
        """(ref, scale) in fp64, [batch][m][n]: alpha * A' . B + beta * C0 and |alpha| * |A'| . |B| + |beta| * |C0|."""
        if pruned not in self._refs:
            m, n, k, batch, nb = self.m, self.n, self.k, self.batch, self.nb
            a = self.pruned_bits(orc) if pruned else self.a_compact()
            A = a.view(np.float32).astype(np.float64).reshape(batch, m, k)
            B = self.b_compact().view(np.float32).astype(np.float64).reshape(nb, k, n)
            prod = np.stack([A[i] @ B[i % nb] for i in range(batch)])
            absprod = np.stack([np.abs(A[i]) @ np.abs(B[i % nb]) for i in range(batch)])
            ref, scale = self.lay.alpha * prod, abs(self.lay.alpha) * absprod
            if self.reads_c:
                c0 = self.C0.view(np.float32).astype(np.float64).reshape(batch, m, n)
                ref, scale = ref + self.lay.beta * c0, scale + abs(self.lay.beta) * np.abs(c0)
            self._refs[pruned] = (ref + 0.0, scale)
        return self._refs[pruned]

    def assert_ties_premise(self, orc, which=(False, True)):
        """Small integers, k <= 256, alpha and beta powers of two: every fp32 product, partial sum, bf16 piece and scale the kernels
        make is exact, so the fp64 result is an fp32 value."""
        assert self.kind == "ties" and self.k <= 256 and (self.lay.alpha, self.lay.beta) in ((1.0, 0.0), AB)
        for pruned in which:
            ref, scale = self.reference(orc, pruned)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and max(np.abs(ref).max(), scale.max()) < 2.0 ** 24

    # ---- device ---------------------------------------------------------------------------------
    def to_device(self):
        self.dA, self.dB, self.dC = (g.to_device().dev for g in (self.gA, self.gB, self.gC))
        return self

    def ptr(self, which):
        return getattr(self, "g" + which).ptr

    def reset_c(self):
        import torch
        self.dC.copy_(torch.from_numpy(self.C.view(np.int32)))

    def result(self, what):
        """The logical C as bits, after asserting that every sentinel outside it kept its bits and that A and B are unchanged."""
        got = self.gC.read()
        if self.lay.gapC and self.batch > 1:
            gap = self.baseC + self.m * self.n + np.arange(self.lay.gapC)
            assert np.array_equal(got[gap], self.C[gap]), f"{what}: the strideC gap behind batch 0 was written (the fold fired on a gap, or b * strideC is wrong)"
        self.gC.assert_outside_kept(lambda n, first: f"{what}: {n} words of C outside the logical result were written, first at {first}", got)
        assert self.gA.unchanged(), f"{what}: A was modified"
        assert self.gB.unchanged(), f"{what}: B was modified"
        return got[self.iC]

    def untouched(self):
        return self.gC.unchanged()

    def check(self, orc, what, entry, got, planes=None):
        ref, scale = self.reference(orc, entry not in ("dense", "dsplit"))
        ref, scale = ref.reshape(-1), scale.reshape(-1)
        g = got.view(np.float32)
        bad = np.flatnonzero(np.isnan(g))
        assert bad.size == 0, (f"{what}: {bad.size} NaN results (padding read into a product?), first at (batch, row, col) "
                               f"{np.unravel_index(bad[:4], (self.batch, self.m, self.n))}")
        if self.kind == "ties":
            wrong = np.flatnonzero(got != bits(ref.astype(np.float32)))
            assert wrong.size == 0, (f"{what}: {wrong.size} results are not the exact product, first at (batch, row, col) "
                                     f"{np.unravel_index(wrong[:4], (self.batch, self.m, self.n))}")
        elif planes is not None:
            ratio = float((np.abs(g.astype(np.float64) - ref) / split_bound(planes, self.k, scale, ref)).max())
            MARGINS.append((what, ratio))
            assert ratio <= 1.0, f"{what}: max err / split bound = {ratio:.3f}"
            assert not (np.abs(g.astype(np.float64) - ref) > FP32_TOL * np.maximum(scale, 1e-30)).any()
        else:
            check_close(g, ref, scale, FP32_TOL, what, self.k, "f32")
            if entry in ("dense", "fused"):   # an exact fmaf chain: far tighter than the 1e-3 the metric asks for
                check_close(g, ref, scale, 1e-5, what + " tight", self.k, "f32")


# ---------------------------------------------------------------------------------------------
# the entry points through the C ABI (pointers as integers: the refusals are called without a device too)
# ---------------------------------------------------------------------------------------------
ENTRIES = ("dense", "fused", "staged", "split", "dsplit", "prep")
TAKES_LDA = ("dense", "fused", "split", "dsplit", "prep")


def call_entry(L, entry, A, B, C, p, planes=3, ws=0, ws_bytes=0, **over):
    """The status of one call on p's layout; A: the dense A (staged: the blob); over: lda / sA / sB / sC replaced."""
    lda, sA, sB, sC = (over.get(x, getattr(p, x)) for x in ("lda", "sA", "sB", "sC"))
    m, n, k, batch, al, be = p.m, p.n, p.k, p.batch, p.lay.alpha, p.lay.beta
    if entry == "dense":
        return L.sm_gemm_rowmajor_f32(A, B, C, m, n, k, lda, batch, sA, sB, sC, al, be, None)
    if entry == "fused":
        return L.sm_spmma_fused_f32(A, B, C, m, n, k, lda, batch, sA, sB, sC, al, be, None)
    if entry == "staged":
        return L.sm_spmma_f32(A, B, C, m, n, k, batch, sB, sC, al, be, None)
    if entry == "split":
        return L.sm_spmma_fused_f32_split(A, B, C, m, n, k, lda, batch, sA, sB, sC, planes, ws, ws_bytes, al, be, None)
    if entry == "dsplit":
        return L.sm_gemm_rowmajor_f32_split(A, B, C, m, n, k, lda, batch, sA, sB, sC, planes, ws, ws_bytes, al, be, None)
    assert entry == "prep"
    return L.sm_spmma_fused_f32_split_prepared(A, ws, C, m, n, k, lda, batch, sA, sB, sC, planes, ws_bytes, al, be, None)


def run(gpu, entry, p, A=None, **kw):
    rc = call_entry(gpu.lib(), entry, p.ptr("A") if A is None else A, p.ptr("B"), p.ptr("C"), p, **kw)
    assert rc == 0, f"{entry}: status {rc}: {gpu.lib().sm_last_error().decode()}"


def workspace(gpu, p, planes):
    import torch
    need = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmma_fused_f32_split_workspace(p.n, p.k, p.batch, p.sB, planes, ctypes.byref(need)) == 0
    return torch.empty(max(16, need.value), dtype=torch.uint8, device="cuda")


def dense_of_pruned_compact(gpu, orc, p):
    """sm_gemm_rowmajor_f32 of the oracle-pruned A on COMPACT copies of the operands: the bits sm_spmma_fused_f32 must return."""
    import torch
    up = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    tail = np.full(GUARD, SENT, dtype=np.uint32)
    dA, dB, dC = up(p.pruned_bits(orc)), up(p.b_compact()), up(np.concatenate([p.C0, tail]))
    rc = gpu.lib().sm_gemm_rowmajor_f32(dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), p.m, p.n, p.k, p.k, p.batch, p.m * p.k, 0 if p.nb == 1 else p.k * p.n,
                                        p.m * p.n, p.lay.alpha, p.lay.beta, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = dC.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[p.C0.size:], tail), "the dense kernel on compact copies wrote past the end of C"
    return got[: p.C0.size]


def run_mm(gpu, orc, p, what, fused=True):
    """sm_gemm_rowmajor_f32 and (fused) sm_spmma_fused_f32, the latter also against the dense kernel of the pruned compact A."""
    run(gpu, "dense", p)
    p.check(orc, f"sm_gemm_rowmajor_f32 {what}", "dense", p.result("dense " + what))
    p.reset_c()
    if fused:
        run(gpu, "fused", p)
        got = p.result("fused " + what)
        p.check(orc, f"sm_spmma_fused_f32 {what}", "fused", got)
        assert np.array_equal(got, dense_of_pruned_compact(gpu, orc, p)), f"fused {what}: differs from sm_gemm_rowmajor_f32 of the oracle-pruned compact A"
        p.reset_c()


def run_staged(gpu, orc, p, what):
    import torch
    blob = torch.from_numpy(orc.compress24(p.a_compact(), p.m, p.k, p.k, p.batch)).cuda()
    assert blob.data_ptr() % 16 == 0
    run(gpu, "staged", p, A=blob.data_ptr())
    p.check(orc, f"sm_spmma_f32 {what}", "staged", p.result("staged " + what))
    p.reset_c()


def run_split(gpu, orc, p, planes, what):
    """Both split forms, and the prepared twin from planes made while B was there: B holds nothing but NaN during the product."""
    import torch
    ws = workspace(gpu, p, planes)
    kw = dict(planes=planes, ws=ws.data_ptr(), ws_bytes=ws.numel())
    run(gpu, "dsplit", p, **kw)
    p.check(orc, f"sm_gemm_rowmajor_f32_split planes {planes} {what}", "dsplit", p.result("dense split " + what), planes)
    p.reset_c()
    ws.fill_(0xFF)
    run(gpu, "split", p, **kw)
    got = p.result("split " + what)
    p.check(orc, f"sm_spmma_fused_f32_split planes {planes} {what}", "split", got, planes)
    p.reset_c()
    ws.fill_(0xFF)
    rc = gpu.lib().sm_spmma_fused_f32_split_prepare(p.ptr("B"), p.n, p.k, p.batch, p.sB, planes, ws.data_ptr(), ws.numel(), None)
    assert rc == 0, gpu.lib().sm_last_error().decode()
    p.dB.view(torch.float32).fill_(float("nan"))
    run(gpu, "prep", p, **kw)
    p.dB.copy_(torch.from_numpy(p.B.view(np.int32)))
    assert np.array_equal(p.result("prepared " + what), got), f"prepared {what}: differs from sm_spmma_fused_f32_split"
    p.reset_c()


# ---------------------------------------------------------------------------------------------
# launch classes: what each needs from a case (test_strided32_cases.py holds every case against this table)
# ---------------------------------------------------------------------------------------------
def facts(fam, m, n, k, lay):
    """What the dispatch looks at, from the layout alone.  M: the rows of one grid batch after the fold."""
    lda, batch = k + lay.lda_pad, lay.batch
    gaps = (lay.gapB is not None, lay.gapC != 0) + ((lay.gapA != 0,) if fam != "staged" else ())
    fold = batch > 1 and not any(gaps)
    sB = 0 if lay.gapB is None else k * n + lay.gapB
    f = dict(fold=fold, M=m * batch if fold else m, N=n, k32=k % 32 == 0 and k >= 32, k64=k % 64 == 0 and k >= 64, n4=n % 4 == 0, n8=n % 8 == 0,
             a16=lda % 4 == 0 and (m * lda + lay.gapA) % 4 == 0 and lay.offA % 4 == 0, b16=sB % 4 == 0 and lay.offB % 4 == 0,
             c16=(m * n + lay.gapC) % 4 == 0 and lay.offC % 4 == 0, tall=batch == 1 or fold, lda_is_k=lay.lda_pad == 0)
    f["dma"] = f["k32"] and f["a16"] and f["b16"] and f["n4"]
    f["pairs"] = f["M"] % 2 == 0
    f["sdma"] = f["k64"] and f["pairs"] and f["n4"] and f["b16"]
    f["small_tiles"] = ((f["M"] + 63) // 64) * ((n + 63) // 64) * (1 if fold else batch)
    return f


# the split forms all need 16-byte aligned bases and strides of A, B and C, n % 8 == 0 and a packed or shared B (`split_ok`)
CLASS_NEEDS = {
    "dma<64,64>": lambda f: f["dma"] and f["M"] <= 64 and f["N"] <= 64 and not f["fold"],
    "dma<64,128>": lambda f: f["dma"] and f["M"] <= 64 and f["N"] > 64 and not f["fold"],
    "dma<128,64>": lambda f: f["dma"] and f["M"] > 64 and f["N"] <= 128,
    "dma<128,128>": lambda f: f["dma"] and f["M"] > 64 and f["N"] > 128,
    "generic<64,64>": lambda f: not f["dma"] and f["small_tiles"] < 32 * 32,       # below 32 tiles per CU from 32 CUs on
    "generic<128,64>": lambda f: not f["dma"] and f["small_tiles"] >= 32 * 256,    # (sized for 256 CUs here; from the device's count on the GPU)
    "staged dma<64,4,1>": lambda f: f["sdma"],
    "staged generic": lambda f: not f["sdma"] and f["small_tiles"] < 32 * 32,
    "split<64>": lambda f: f["split_ok"] and f["a16"] and f["k64"] and f["N"] <= 64,
    "split<128> ant": lambda f: f["split_ok"] and f["a16"] and f["k64"] and 64 < f["N"] <= 128,
    "split cols": lambda f: f["split_ok"] and f["a16"] and f["k64"] and 128 < f["N"] <= 256,
    "split<128> nt": lambda f: f["split_ok"] and f["a16"] and f["k64"] and f["N"] > 256,
    "span<64>": lambda f: f["span_fits"] and f["split_ok"] and not f["k64"] and f["tall"] and f["lda_is_k"] and f["span_bytes16"] and f["N"] <= 64,
    "span<128>": lambda f: f["span_fits"] and f["split_ok"] and not f["k64"] and f["tall"] and f["lda_is_k"] and f["span_bytes16"] and 64 < f["N"] <= 128,
}


def case_facts(c):
    lay = layout_of(c.fam, c.lname)
    f = facts(c.fam, c.m, c.n, c.k, lay)
    f["split_ok"] = (lay.offA % 4 == 0 and (c.m * (c.k + lay.lda_pad) + lay.gapA) % 4 == 0 and f["n8"] and f["b16"] and f["c16"] and lay.gapB in (None, 0)
                     and (f["a16"] or lay.lda_pad == 0))          # rows of whole 16-byte chunks, or (the span form) lda == k
    f["span_bytes16"] = (c.m * lay.batch * c.k * 4) % 16 == 0
    f["span_fits"] = span_fits(c.n, c.k, c.planes or 3)
    return f


def span_fits(n, k, planes):
    """include/sparsifyme.h: the span of 128 rows (whole KiB, 256 bytes of slack) and B's planes, k rounded up to 64, inside 160 KiB of LDS."""
    return (128 * k * 4 + 256 + 1023) // 1024 * 1024 + planes * ((k + 63) // 64 * 64) * (64 if n <= 64 else 128) * 2 <= 160 * 1024


# ---------------------------------------------------------------------------------------------
# matmul cases: launch class x layout
# ---------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "fam cls m n k lname planes", defaults=(None,))
M = 200                                # one full 128-row tile plus a ragged one
KS_MM = (32, 64, 160)                  # one stage, exactly the ring depth, odd and longer
KS_64 = (64, 192)                      # one 64-k stage (the LDS is sized for one), more than one
FOLDING = ("compact", "lda+4", "lda+16", "off16", "c_off1", "tall", "ab")
PER_BATCH = ("sA+64", "sB+16", "sB=kn", "sC+8", "sC+3", "all")


def _walk(shapes, layouts_of, ks, fam, planes=(None,)):
    """Every k on `all` and `tall`; the other layouts walk the k's per shape."""
    out = []
    for j, (cls, m, n) in enumerate(shapes):
        for i, lname in enumerate(layouts_of(m)):
            for k in (ks if lname in ("all", "tall") else (ks[(i + j) % len(ks)],)):
                out += [Case(fam, cls, m, n, k, lname, pl) for pl in planes]
    return out


MM_CASES = _walk([("dma<64,64>", 40, 40), ("dma<64,128>", 40, 72), ("dma<64,128>", 40, 200), ("dma<128,64>", M, 40), ("dma<128,64>", M, 104),
                  ("dma<128,128>", M, 136)], lambda m: PER_BATCH if m <= 64 else FOLDING + PER_BATCH, KS_MM, "mm")
# the register-staged kernel, reached each way separately; dense only (the fused form refuses these: REFUSALS)
GENERIC_CASES = [Case("mm", "generic<64,64>", M, n, k, lname) for n, k, lname in
                 [(40, 72, "compact"), (37, 64, "compact"), (40, 64, "lda+1"), (40, 64, "sA+2"), (40, 64, "a_off1"), (40, 64, "b_off1"), (40, 5, "compact"),
                  (37, 72, "all"), (37, 72, "tall"), (40, 72, "sC+3"), (37, 5, "ab"), (40, 5, "lda+1"), (136, 72, "sC+8")]]
STAGED_LAYOUTS = ("compact", "sB+16", "sB=kn", "sC+8", "sC+3", "c_off1", "off16", "tall", "ab", "all")
STAGED_CASES = _walk([("staged dma<64,4,1>", M, 40), ("staged dma<64,4,1>", M, 104)], lambda m: STAGED_LAYOUTS, KS_64, "staged")
STAGED_CASES += [Case("staged", "staged generic", m, n, k, lname) for m, n, k, lname in
                 [(M, 40, 72, "compact"), (M, 37, 64, "compact"), (201, 40, 64, "sC+8"), (201, 40, 64, "tall"), (M, 40, 64, "b_off1"), (M, 40, 64, "sB+2"),
                  (201, 37, 72, "all"), (M, 37, 72, "ab"), (M, 37, 64, "sC+3"), (M, 40, 72, "sB+16")]]
SPLIT_LAYOUTS = ("compact", "lda+4", "lda+16", "sA+64", "sB=kn", "sC+8", "off16", "tall", "ab", "all")
SPLIT_CASES = _walk([("split<64>", M, 40), ("split<128> ant", M, 104), ("split cols", M, 136), ("split cols", M, 256), ("split<128> nt", M, 264)],
                    lambda m: SPLIT_LAYOUTS, KS_64, "split", (2, 3))
# the span form (ragged k): one tall contiguous A, batch 3; m * batch * k * 4 is a multiple of 16 and m no multiple of 128
# (k = 147 with n = 104 does not fit: span + planes need 170 / 218 KiB of LDS for planes = 2 / 3, the header's NOT_SUPPORTED: REFUSALS)
SPLIT_CASES += [Case("split", "span<64>" if n <= 64 else "span<128>", M, n, k, lname, pl) for k in (72, 147) for n in (40, 104) for lname in ("tall", "tall+off16")
                for pl in (2, 3) if span_fits(n, k, pl)]
ALL_CASES = MM_CASES + GENERIC_CASES + STAGED_CASES + SPLIT_CASES


def _cid(c):
    return "-".join(str(x) for x in c if x is not None)


def problems(c):
    """The case's problem, once per data kind."""
    for kind in KINDS:
        yield Problem(c.m, c.n, c.k, layout_of(c.fam, c.lname), kind, np.random.default_rng(_seed(kind, *(x for x in c if x is not None))))


@pytest.mark.parametrize("case", MM_CASES + GENERIC_CASES, ids=_cid)
def test_dense_and_fused_on_padded_operands(gpu, orc, case):
    for p in problems(case):
        if p.kind == "ties":
            p.assert_ties_premise(orc)
        run_mm(gpu, orc, p.to_device(), f"{p.kind} {_cid(case)}", fused=not case.cls.startswith("generic"))


@pytest.mark.parametrize("case", STAGED_CASES, ids=_cid)
def test_staged_on_padded_operands(gpu, orc, case):
    for p in problems(case):
        if p.kind == "ties":
            p.assert_ties_premise(orc)
        run_staged(gpu, orc, p.to_device(), f"{p.kind} {_cid(case)}")


@pytest.mark.parametrize("case", SPLIT_CASES, ids=_cid)
def test_split_forms_on_padded_operands(gpu, orc, case):
    for p in problems(case):
        if p.kind == "ties":
            p.assert_ties_premise(orc)
        run_split(gpu, orc, p.to_device(), case.planes, f"{p.kind} {_cid(case)}")


# ---- both sides of every tile threshold, the smaller problem a corner of the larger one's operands
# (family, which extent, the two values, the fixed extents, k, whether the class changes).  N <= 64 decides only when M <= 64
# (gemm_f32.hip:609): crossed at m = 40; n = 64 / 68 at m = 200 stays in dma<128,64> on both sides and is kept as a ragged-n pair.
THRESHOLDS = [("mm", "m", (64, 68), dict(n=40), 160, True), ("mm", "n", (64, 68), dict(m=40), 160, True), ("mm", "n", (64, 68), dict(m=M), 160, False),
              ("mm", "n", (128, 132), dict(m=M), 160, True), ("split", "n", (64, 72), dict(m=M), 192, True), ("split", "n", (128, 136), dict(m=M), 192, True),
              ("split", "n", (256, 264), dict(m=M), 192, True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("thr", THRESHOLDS, ids=lambda t: f"{t[0]}-{t[1]}-{t[2][0]}-{t[2][1]}-{t[3]}".replace("'", "").replace(": ", "").replace("{", "").replace("}", ""))
def test_both_sides_of_each_threshold(gpu, orc, thr, kind):
    fam, ext, vals, fixed, k, _ = thr
    lay = layout_of(fam, "all")
    big = dict(fixed, **{ext: max(vals)})
    a, b, c0 = draw(np.random.default_rng(_seed("thr", fam, ext, *vals, kind)), kind, lay.batch, lay.batch, big["m"], big["n"], k)
    for v in vals:
        d = dict(fixed, **{ext: v})
        m, n = d["m"], d["n"]
        p = Problem(m, n, k, lay, kind, data=(a[:, :m], b[:, :, :n], c0[:, :m, :n]))
        if kind == "ties":
            p.assert_ties_premise(orc)
        p.to_device()
        if fam == "mm":
            run_mm(gpu, orc, p, f"{kind} threshold {ext}={v}")
        else:
            for planes in (2, 3):
                run_split(gpu, orc, p, planes, f"{kind} threshold {ext}={v}")


# ---- the register-staged kernel's 128 x 64 tiling: taken from 32 64 x 64 tiles per CU on, which no shape of the suite reached
def big_generic_shape(cus, per_batch):
    """(m, n, k, layout name): ceil(m / 64) * 2 * batch = 32 * cus small tiles, a thin k that is no multiple of 32, n % 64 != 0."""
    rows = (32 * cus + 1) // 2 * 64
    return ((rows + 1) // 2, 72, 20, "sA+64") if per_batch else (rows // 2, 72, 20, "compact")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per_batch", [False, True], ids=["folded", "sA+64"])
def test_dense_generic_128x64_tiles(gpu, orc, per_batch, kind):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, n, k, lname = big_generic_shape(cus, per_batch)
    lay = layout_of("mm", lname)
    f = facts("mm", m, n, k, lay)
    assert not f["dma"] and f["fold"] != per_batch and f["small_tiles"] / cus >= 32.0, "the case does not reach launch32<128, 64, 4, 1, 0>"
    p = Problem(m, n, k, lay, kind, np.random.default_rng(_seed("big", per_batch, kind)))
    assert (p.A.size + p.B.size + p.C.size) * 4 < 150e6 * max(1.0, cus / 256.0)
    if kind == "ties":
        p.assert_ties_premise(orc, which=(False,))
    run_mm(gpu, orc, p.to_device(), f"{kind} generic<128,64> {lname} (m, n, k) = {(m, n, k)}", fused=False)


# ---------------------------------------------------------------------------------------------
# refusals: decided before any device work, C untouched
# ---------------------------------------------------------------------------------------------
SPLITS = ("split", "dsplit", "prep")
# name -> (entries, layout name, overrides of the call, k, status[, n])
REFUSALS = {
    "fused lda+1": (("fused",), "lda+1", {}, 64, NOT_SUPPORTED),
    "fused sA+2": (("fused",), "sA+2", {}, 64, NOT_SUPPORTED),
    "fused sB+2": (("fused",), "sB+2", {}, 64, NOT_SUPPORTED),
    "fused a_off1": (("fused",), "a_off1", {}, 64, NOT_SUPPORTED),
    "fused b_off1": (("fused",), "b_off1", {}, 64, NOT_SUPPORTED),
    "split sC+3": (SPLITS, "sC+3", {}, 64, NOT_SUPPORTED),
    "split c_off1": (SPLITS, "c_off1", {}, 64, NOT_SUPPORTED),
    "split sB+16": (SPLITS, "sB+16", {}, 64, NOT_SUPPORTED),             # a strided B must be packed
    "split ragged k lda+4": (SPLITS, "lda+4", {}, 72, NOT_SUPPORTED),    # the span form needs lda == k ...
    "split ragged k sA+64": (SPLITS, "sA+64", {}, 72, NOT_SUPPORTED),    # ... and one tall contiguous A
    "split span k=147 n=104": (SPLITS, "tall", {}, 147, NOT_SUPPORTED, 104),  # the span and B's planes do not fit the LDS (planes 2 or 3)
    "lda<k": (TAKES_LDA, "compact", dict(lda=60), 64, INVALID),
}
REFUSAL_MN = (M, 40)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_c_alone(gpu, name):
    entries, lname, over, k, status = REFUSALS[name][:5]
    p = Problem(REFUSAL_MN[0], (REFUSALS[name] + (REFUSAL_MN[1],))[5], k, Layout(**LAYOUTS[lname]), "uniform", np.random.default_rng(_seed(name))).to_device()
    ws = workspace(gpu, p, 3)
    for entry in entries:
        for planes in (2, 3):
            rc = call_entry(gpu.lib(), entry, p.ptr("A"), p.ptr("B"), p.ptr("C"), p, planes=planes, ws=ws.data_ptr(), ws_bytes=ws.numel(), **over)
            assert rc == status, f"{name} {entry} planes {planes}: status {rc}, not {status}"
            assert p.untouched(), f"{name} {entry}: a refused call wrote to C"


# ---------------------------------------------------------------------------------------------
# margins of this file's `uniform` comparisons, appended to the session's report: the worst per entry point, then the worst cases
# ---------------------------------------------------------------------------------------------
_strided32_margin_report = margin_report_fixture(
    "{n} comparisons of tests/test_gpu_strided32.py against the numpy fp64 product; err / bound (check_close; split forms: split_bound), "
    "worst per entry point:", per_first_word=True)
