"""The 16-bit 2:4 and dense matmuls on PADDED operands, per kernel form (-m gpu).

Every case places the logical operands in larger buffers (a base offset, lda > k, gaps in the batch strides): all of A and B outside
the logical operand is NaN, all of C outside the logical result a sentinel bit pattern.  A kernel that reads padding into a product
shows a NaN; one that writes outside its tile changes a sentinel; a wrong row base shows in the integer-exact variant.  The
reference is NOT the library: the gathered logical A, pruned by the oracle's STRIP rule on the compact copy, times B in numpy fp64,
under exactly parity_testlib.check_close's bound (imported, not restated).  Every exact fused form is also held, bit for bit,
against compress + sm_spmma_* on a compact copy -- the library's stated contract.

Each fused case FIRST asserts, through sm_spmma_fused_form with cus = 0, that this device sends the call to the form the case is
pinned to (FUSED_CASES; the same table is checked at 256 CUs without a GPU by test_fused_form_abi.py): a case that reaches another
kernel fails, it never skips."""
import numpy as np
import pytest

import parity_testlib as pl
from guard_testlib import Guarded, Layout, Strided, dev_bits, f64_of as _f64_of, host_bits, margin_report_fixture, round_bits as _round_bits, seed
from parity_testlib import FP16_TOL, check_close   # the one bound: ROUND*|ref| + 2k*ACC*sum|ab| + TINY, and the 1e-2 north star

pytestmark = pytest.mark.gpu

NAN_BITS = {False: 0x7E00, True: 0x7FC0}     # a quiet NaN of f16 / bf16
SENTINEL = 0x5A5A                            # finite in both types; no product of these tests rounds to it by design of the check
DT = [False, True]
DT_IDS = ["f16", "bf16"]


# ---------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------
def rand_bits(rng, n, bf, kind="uniform"):
    if bf:
        return pl.bf16_bits(rng, n, kind)
    return pl.bits(pl.rand(rng, n, np.float16, kind)).copy()


def f64_of(b, bf):
    return _f64_of(b, DT_IDS[bf])


def bits_of_f64(x, bf):
    """Exactly representable values (small integers) as bit patterns."""
    import torch
    if bf:
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
    return np.ascontiguousarray(x, dtype=np.float16).view(np.uint16).copy()


def round_bits(x, bf):
    return _round_bits(x, DT_IDS[bf])


def dev(b, bf):
    return dev_bits(b, DT_IDS[bf])


# ---------------------------------------------------------------------------------------------
# the layout builder
# ---------------------------------------------------------------------------------------------
class Problem(Strided):
    """Padded host buffers (bit patterns), index maps of the logical operands, the fp64 reference and -- after to_device(), which the
    constructor calls unless told upload=False -- the device copies."""

    def __init__(self, rng, m, n, k, lay, bf, kind="uniform", int_b=False, dense=False, slack_rows=256, upload=True):
        Strided.__init__(self, m, n, k, lay, lay.offA, lay.offB, lay.offC)
        self.bf = bf
        batch, nb, lda = self.batch, self.nb, self.lda
        # whole-tile reads past a ragged m (and 16-byte pieces past a row's end) stay inside the allocations
        self.gA = Guarded(lay.offA + batch * self.sA + slack_rows * lda + 64, NAN_BITS[bf], np.uint16, lay.offA, self.iA)
        self.gB = Guarded(lay.offB + nb * self.sBe + 64 * n + 64, NAN_BITS[bf], np.uint16, lay.offB, self.iB)
        self.gC = Guarded(lay.offC + batch * self.sC + 64, SENTINEL, np.uint16, lay.offC, self.iC)
        self.A, self.B, self.C = self.gA.host, self.gB.host, self.gC.host
        self.A[self.iA] = rand_bits(rng, batch * m * k, bf, kind)
        if int_b:   # asymmetric small integers, as test_mfma_lane_maps_with_identity_and_asymmetric_b's B
            Bi = ((np.arange(k)[:, None] * 3 + np.arange(n)[None, :] * 7) % 13 - 6).astype(np.float64)
            self.B[self.iB] = np.concatenate([bits_of_f64(Bi + b, bf).reshape(-1) for b in range(nb)])
        else:
            self.B[self.iB] = rand_bits(rng, nb * k * n, bf)
        self.C0 = rand_bits(rng, batch * m * n, bf) if lay.beta != 0.0 else np.full(batch * m * n, SENTINEL, dtype=np.uint16)
        self.C[self.iC] = self.C0
        self.dense = dense
        if upload:
            self.to_device()

    def to_device(self):
        import torch
        lay, ty = self.lay, torch.bfloat16 if self.bf else torch.float16
        self.dA, self.dB, self.dC = (g.to_device().dev.view(ty) for g in (self.gA, self.gB, self.gC))
        self.pA, self.pB, self.pC = self.dA[lay.offA:], self.dB[lay.offB:], self.dC[lay.offC:]
        return self

    def a_compact(self):
        return self.A[self.iA].copy()

    def b_compact(self):
        return self.B[self.iB].copy()

    def reference(self, orc):
        """(ref, scale) in fp64: alpha * P @ B + beta * C0 with P the oracle's STRIP prune of the compact A (dense: P = A)."""
        m, n, k, batch, bf, lay = self.m, self.n, self.k, self.batch, self.bf, self.lay
        Ac = self.a_compact()
        Pb = Ac if self.dense else orc.prune24(Ac, batch * m, k, k, orc.STRIP, bf16=bf)
        P = f64_of(Pb, bf).reshape(batch, m, k)
        Bm = f64_of(self.b_compact(), bf).reshape(self.nb, k, n)
        C0 = f64_of(self.C0, bf).reshape(batch, m, n) if lay.beta != 0.0 else np.zeros((batch, m, n))
        ref = np.stack([lay.alpha * (P[b] @ Bm[b % self.nb]) + lay.beta * C0[b] for b in range(batch)])
        scale = np.stack([abs(lay.alpha) * (np.abs(P[b]) @ np.abs(Bm[b % self.nb])) + abs(lay.beta) * np.abs(C0[b]) for b in range(batch)])
        return ref.reshape(-1), scale.reshape(-1)

    def result(self):
        """The logical C as bits, after asserting that every sentinel outside it kept its bits."""
        return self.gC.result(lambda n, first: f"{n} elements of C outside the logical result were written, first at {first}")

    def check(self, orc, what, exact=False):
        got = self.result()
        g64 = f64_of(got, self.bf)
        bad = np.flatnonzero(~np.isfinite(g64))
        assert bad.size == 0, f"{what}: {bad.size} non-finite results (padding read into a product?), first at (batch, row, col) {np.unravel_index(bad[:4], (self.batch, self.m, self.n))}"
        ref, scale = self.reference(orc)
        if exact:   # integer operands: every fp32 product and sum is exact, so the output is the ONE rounding of the exact result
            wrong = np.flatnonzero(g64 != f64_of(round_bits(ref, self.bf), self.bf))
            assert wrong.size == 0, f"{what}: {wrong.size} integer results differ, first at (batch, row, col) {np.unravel_index(wrong[:4], (self.batch, self.m, self.n))}"
        check_close(g64, ref, scale, FP16_TOL, what, self.k, "bf16" if self.bf else "f16")
        return got

    def staged_bits(self, gpu, epilogue=None):
        """compress + sm_spmma_* on compact copies of the same operands: the bits every exact fused form must return."""
        import torch
        m, n, k, batch, bf, lay = self.m, self.n, self.k, self.batch, self.bf, self.lay
        dAc, dBc, dCc = dev(self.a_compact(), bf), dev(self.b_compact(), bf), dev(self.C0.copy(), bf)
        blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
        gpu.compress24(dAc, m, k, k, batch, m * k, blob)
        gpu.spmma(blob, dBc, dCc, m, n, k, batch, 0 if self.nb == 1 else k * n, alpha=lay.alpha, beta=lay.beta, epilogue=epilogue)
        return host_bits(dCc)

    def form(self, gpu, count=1, workspace=False, epilogue=False, cus=0):
        return gpu.spmma_fused_form(self.m, self.n, self.k, self.lda, self.batch, count, self.sA, self.sB, self.sC, self.lay.beta,
                                    a_aligned=self.pA.data_ptr() % 16 == 0, b_aligned=self.pB.data_ptr() % 16 == 0, c_aligned=self.pC.data_ptr() % 16 == 0,
                                    workspace=workspace, epilogue=epilogue, cus=cus)

    def run_fused(self, gpu, **kw):
        lay = self.lay
        gpu.spmma_fused(self.pA, self.pB, self.pC, self.m, self.n, self.k, lda=self.lda, batch=self.batch, strideA=self.sA, strideB=self.sB, strideC=self.sC,
                        alpha=lay.alpha, beta=lay.beta, **kw)


# ---------------------------------------------------------------------------------------------
# the fused forms: one small shape per form (ragged m; n % 8 == 0 and not a multiple of the column tile), every layout
# ---------------------------------------------------------------------------------------------
# form at 256 CUs of the shape with beta == 0 and an aligned C -> (m, n, k)
FORM_SHAPES = {
    "direct64": (200, 40, 128),
    "direct128": (200, 104, 192),
    "direct128_nt": (200, 104, 576),
    "big": (50, 200, 128),
    "astat": (200, 264, 128),
    "widep": (200, 200, 128),
    "wide": (200, 264, 1088),
    "wide_nt": (200, 200, 1088),
}
LAYOUTS = {
    "lda+8": dict(lda_pad=8),
    "lda+64": dict(lda_pad=64),
    "sA+64": dict(gapA=64),
    "sC+8": dict(gapC=8),
    "sC+3": dict(gapC=3),                      # batch 1's C is off a 16-byte boundary: the per-element store
    "sB+8": dict(gapB=8),                      # per-batch B
    "c_off1": dict(offC=1),                    # C base off by one element, beta == 0
    "ab_gapC": dict(gapC=8, alpha=0.5, beta=-2.0),
    "off8": dict(offA=8, offB=8),              # still 16-byte aligned
    "all": dict(lda_pad=8, gapA=64, gapB=8, gapC=8, offA=8, offB=8),
}
# Where a layout moves the shape to ANOTHER form (the A-stationary kernel stores 16-byte pieces of an aligned C with beta == 0 only:
# its shape then runs the persistent wide kernel) -- pinned, asserted on the device, and run all the same.
FORM_MOVES = {("astat", "sC+3"): "widep", ("astat", "c_off1"): "widep", ("astat", "ab_gapC"): "widep"}
FUSED_CASES = [(FORM_MOVES.get((f, l), f), f, l) for f in FORM_SHAPES for l in LAYOUTS]
# span and thin need one tall contiguous A: batch == 1 with the B- and C-side cases and the offsets
TALL_SHAPES = {"span": (200, 72, 200), "thin": (200, 3, 18)}
TALL_LAYOUTS = {
    "plain": dict(batch=1),
    "sC+8": dict(batch=1, gapC=8),             # (one batch: strideC is passed but never read -- this case guards the sentinels only)
    "offB8": dict(batch=1, offB=8),            # the B side: its base moved alone
    "ab": dict(batch=1, alpha=0.5, beta=-2.0),
    "off8": dict(batch=1, offA=8, offB=8, offC=8),
    "stacked": dict(batch=3),
    "c_off1": dict(batch=1, offC=1),           # the thin form stores element-wise; the span form refuses (REFUSALS)
}
TALL_CASES = [(f, f, l) for f in TALL_SHAPES for l in TALL_LAYOUTS if (f, l) != ("span", "c_off1")]


def _case_id(c):
    return "%s-%s" % (c[1], c[2])


def _seed(*xs):
    return seed(0x5716, *xs)


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", FUSED_CASES, ids=_case_id)
def test_fused_form_on_padded_operands(gpu, orc, case, bf):
    form, shape_of, lname = case
    m, n, k = FORM_SHAPES[shape_of]
    p = Problem(np.random.default_rng(_seed(shape_of, lname, bf)), m, n, k, Layout(**LAYOUTS[lname]), bf)
    assert p.form(gpu) == form, f"this device sends {shape_of} / {lname} to another form than the case is pinned to"
    p.run_fused(gpu)
    got = p.check(orc, f"strided fused {form} {lname} {DT_IDS[bf]}")
    assert np.array_equal(got, p.staged_bits(gpu)), f"{form} / {lname}: differs from compress + spmma on the compact copy"


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", TALL_CASES, ids=_case_id)
def test_fused_tall_forms_on_padded_operands(gpu, orc, case, bf):
    form, shape_of, lname = case
    m, n, k = TALL_SHAPES[shape_of]
    p = Problem(np.random.default_rng(_seed(shape_of, lname, bf)), m, n, k, Layout(**TALL_LAYOUTS[lname]), bf, kind="ties" if lname == "ab" else "uniform")
    assert p.form(gpu) == form
    p.run_fused(gpu)
    got = p.check(orc, f"strided fused {form} {lname} {DT_IDS[bf]}")
    if form != "thin":   # (the thin form is inside the bound, not the staged pair's bits: include/sparsifyme.h)
        assert np.array_equal(got, p.staged_bits(gpu)), f"{form} / {lname}: differs from compress + spmma on the compact copy"


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("form", list(FORM_SHAPES) + list(TALL_SHAPES))
def test_fused_form_integer_exact(gpu, orc, form, bf):
    """Small integers in A ("ties") and an asymmetric integer B, different per batch: every product and sum is exact in fp32, so
    the output must EQUAL the fp64 product rounded once to the output type -- a wrong row base or batch offset cannot hide inside a
    tolerance."""
    tall = form in TALL_SHAPES
    m, n, k = (TALL_SHAPES if tall else FORM_SHAPES)[form]
    lay = Layout(batch=1, offA=8, offB=8, offC=8) if tall else Layout(lda_pad=8, gapA=64, gapB=8, gapC=8)
    p = Problem(np.random.default_rng(_seed(form, "int", bf)), m, n, k, lay, bf, kind="ties", int_b=True)
    assert p.form(gpu) == form
    p.run_fused(gpu)
    p.check(orc, f"strided fused integer {form} {DT_IDS[bf]}", exact=True)


# ---------------------------------------------------------------------------------------------
# what the rule refuses: SM_STATUS_NOT_SUPPORTED, C untouched
# ---------------------------------------------------------------------------------------------
REFUSALS = {
    "lda%8_k%64": ((200, 104, 192), dict(lda_pad=4)),
    "sA%8": ((200, 104, 192), dict(gapA=4)),
    "sB%8": ((200, 104, 192), dict(gapB=4)),
    "A_unaligned": ((200, 104, 192), dict(offA=4)),
    "A_unaligned_wide": ((200, 264, 128), dict(offA=4)),
    "span_c_off1": ((200, 72, 200), dict(batch=1, offC=1)),
    "span_lda": ((200, 72, 200), dict(batch=1, lda_pad=8)),
}


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", list(REFUSALS))
def test_fused_refuses_and_leaves_c_alone(gpu, name, bf):
    import torch
    (m, n, k), lay = REFUSALS[name]
    p = Problem(np.random.default_rng(_seed(name, bf)), m, n, k, Layout(**lay), bf)
    assert p.form(gpu) == "not_taken"
    with pytest.raises(gpu.SparsifymeError, match="status 2"):
        p.run_fused(gpu)
    assert np.array_equal(host_bits(p.dC), p.C), "a refused call wrote to C"
    # the prune-in-place + multiply entry point asks the same rule BEFORE it touches A (sm::spmma_fused16_takes_exact); n > 128 or a
    # ragged k keep its own one-kernel form out of the way
    if n > 128 or k % 64:
        Aout = p.dA.clone()
        rc = gpu.prune24_spmma(p.pA, Aout[p.lay.offA:], p.pB, p.pC, m, n, k, lda=p.lda, batch=p.batch, strideA=p.sA, strideB=p.sB, strideC=p.sC,
                               alg=gpu.PRUNE_STRIP, check=False)
        assert rc == gpu.STATUS_NOT_SUPPORTED
        assert torch.equal(Aout.view(torch.int16), p.dA.view(torch.int16)) and np.array_equal(host_bits(p.dC), p.C)


# ---------------------------------------------------------------------------------------------
# the same layouts through the other fused entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("form", list(FORM_SHAPES))
def test_fused_grouped_on_padded_operands(gpu, orc, form, bf):
    """sm_spmma_fused_*_grouped, count 3: padded A (lda, strideA gap), per-batch B, a C gap per problem."""
    m, n, k = FORM_SHAPES[form]
    ps = [Problem(np.random.default_rng(_seed(form, "grp", i, bf)), m, n, k, Layout(lda_pad=8, gapA=64, gapB=8, gapC=8), bf) for i in range(3)]
    assert ps[0].form(gpu, count=3) == form, "this device sends the grouped launch to another form"
    p = ps[0]
    gpu.spmma_fused_grouped([q.pA for q in ps], [q.pB for q in ps], [q.pC for q in ps], m, n, k, lda=p.lda, batch=p.batch, strideA=p.sA, strideB=p.sB,
                            strideC=p.sC)
    for i, q in enumerate(ps):
        got = q.check(orc, f"strided grouped {form} problem {i} {DT_IDS[bf]}")
        assert np.array_equal(got, q.staged_bits(gpu)), f"grouped {form}, problem {i}: differs from compress + spmma"


STREAMK_SHAPE = (100, 264, 2304, 3)


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
def test_fused_streamk_integer_exact(gpu, orc, bf):
    """The stream-K form has tile offsets of its own (32-bit, built from lda) and a fix-up store of its own, and is not bit-identical
    to the staged pair -- so the integer variant is its exact check: integer partial sums are exact in fp32 in whatever order the
    fix-up adds them, and the output must EQUAL the fp64 product rounded once."""
    import torch
    m, n, k, batch = STREAMK_SHAPE
    p = Problem(np.random.default_rng(_seed("sk", "int", bf)), m, n, k, Layout(lda_pad=8, gapA=64, gapB=8, gapC=8, batch=batch), bf, kind="ties", int_b=True)
    assert p.form(gpu, workspace=True) == "streamk"
    ws = pl._sk_ws(gpu)
    p.run_fused(gpu, workspace=ws)
    torch.cuda.synchronize()
    assert pl._sk_ran(ws), "the stream-K kernel did not run"
    assert gpu.spmma_fused_workspace_state(ws) == 0
    p.check(orc, f"strided stream-K integer {DT_IDS[bf]}", exact=True)


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
def test_fused_streamk_on_padded_operands(gpu, orc, bf, ab):
    """sm_spmma_fused_*_ws on a stream-K shape with lda > k and a strideA gap (so the batches are NOT stacked) and a C gap: the
    partial sums of a cut tile are added in another order than the staged kernels', so the oracle bound is the check."""
    import torch
    m, n, k, batch = STREAMK_SHAPE
    p = Problem(np.random.default_rng(_seed("sk", bf, ab[1] != 0)), m, n, k, Layout(lda_pad=8, gapA=64, gapC=8, batch=batch, alpha=ab[0], beta=ab[1]), bf)
    assert p.form(gpu, workspace=True) == "streamk"
    ws = pl._sk_ws(gpu)
    p.run_fused(gpu, workspace=ws)
    torch.cuda.synchronize()
    assert pl._sk_ran(ws), "the stream-K kernel did not run"
    assert gpu.spmma_fused_workspace_state(ws) == 0
    p.check(orc, f"strided stream-K {ab} {DT_IDS[bf]}")


EX_SHAPES = {"direct128": (200, 104, 192), "big": (100, 200, 128), "wide": (200, 264, 128), "wide_nt": (200, 200, 128)}


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("bias_dim", ["col", "row"])
@pytest.mark.parametrize("form", list(EX_SHAPES))
def test_fused_and_staged_ex_on_padded_operands(gpu, orc, form, bias_dim, bf):
    """sm_spmma_fused_*_ex and sm_spmma_*_ex: a strideD gap with a residual whose strideR has ANOTHER gap, a bias and relu; with an
    epilogue the A-stationary and persistent wide shapes run the wide kernels."""
    import torch
    m, n, k = EX_SHAPES[form]
    alpha, beta, gapR = 0.5, -2.0, 24
    rng = np.random.default_rng(_seed(form, "ex", bias_dim, bf))
    p = Problem(rng, m, n, k, Layout(lda_pad=8, gapA=64, gapB=8, gapC=8, alpha=alpha), bf)   # (D itself is not read: its sentinels stay)
    batch, sR = p.batch, m * n + gapR
    R = np.full(batch * sR + 64, NAN_BITS[bf], dtype=np.uint16)
    iR = (np.arange(batch)[:, None] * sR + np.arange(m * n)[None, :]).reshape(-1)
    R[iR] = rand_bits(rng, batch * m * n, bf)
    bias = rng.uniform(-1, 1, n if bias_dim == "col" else m).astype(np.float32)
    dR, dbias = dev(R, bf), torch.from_numpy(bias).cuda()
    ep = gpu.Epilogue(bias=dbias, bias_dim=bias_dim, act="relu", residual=dR, stride_residual=sR)
    lay = p.lay
    fq = gpu.spmma_fused_form(m, n, k, p.lda, batch, 1, p.sA, p.sB, p.sC, beta, epilogue=True)
    assert fq == form, "this device sends the epilogue call to another form"
    gpu.spmma_fused(p.pA, p.pB, p.pC, m, n, k, lda=p.lda, batch=batch, strideA=p.sA, strideB=p.sB, strideC=p.sC, alpha=alpha, beta=beta, epilogue=ep)
    got = p.result()
    # reference: act(alpha * P @ B + beta * R + bias) in fp64
    P = f64_of(orc.prune24(p.a_compact(), batch * m, k, k, orc.STRIP, bf16=bf), bf).reshape(batch, m, k)
    Bm = f64_of(p.b_compact(), bf).reshape(batch, k, n)
    R64 = f64_of(R[iR], bf).reshape(batch, m, n)
    b64 = bias.astype(np.float64)[None, None, :] if bias_dim == "col" else bias.astype(np.float64)[None, :, None]
    pre = alpha * np.einsum("bmk,bkn->bmn", P, Bm) + beta * R64 + b64
    scale = abs(alpha) * np.einsum("bmk,bkn->bmn", np.abs(P), np.abs(Bm)) + abs(beta) * np.abs(R64) + np.abs(b64)
    check_close(f64_of(got, bf), np.maximum(pre, 0.0).reshape(-1), scale.reshape(-1), FP16_TOL, f"strided fused ex {form} {bias_dim} {DT_IDS[bf]}", k,
                "bf16" if bf else "f16")
    # the staged _ex on the same padded B / D / R must give the same bits
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dev(p.a_compact(), bf), m, k, k, batch, m * k, blob)
    q = Problem(np.random.default_rng(1), m, n, k, Layout(gapB=8, gapC=8, alpha=alpha), bf)
    q.dB.copy_(p.dB[p.lay.offB:][:q.dB.numel()])
    gpu.spmma(blob, q.pB, q.pC, m, n, k, batch, q.sB, q.sC, alpha=alpha, beta=beta, epilogue=ep)
    assert np.array_equal(q.result(), got), "sm_spmma_*_ex and sm_spmma_fused_*_ex differ on the padded operands"


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("alg", ["TILE", "STRIP"])
@pytest.mark.parametrize("shape", [(200, 104, 192), (200, 264, 128)], ids=["one_kernel", "prune_then_fused"])
def test_prune24_spmma_on_padded_operands(gpu, orc, shape, alg, bf):
    """sm_prune24_spmma_* with lda > k and a strideA gap: A_out equals the oracle's prune inside the m x k region, its padding and
    gap keep their bits, C is inside the bound of (pruned A) x B."""
    m, n, k = shape
    algn = getattr(orc, alg)
    p = Problem(np.random.default_rng(_seed("ps", m, n, alg, bf)), m, n, k, Layout(lda_pad=8, gapA=64, gapC=8), bf, kind="ties" if alg == "TILE" else "uniform")
    Aout = dev(np.full(p.A.size, SENTINEL, dtype=np.uint16), bf)
    gpu.prune24_spmma(p.pA, Aout, p.pB, p.pC, m, n, k, lda=p.lda, batch=p.batch, strideA=p.sA, strideB=p.sB, strideC=p.sC, alg=algn)
    want = np.full(p.A.size, SENTINEL, dtype=np.uint16)
    Pb = orc.prune24(p.a_compact(), p.batch * m, k, k, algn, bf16=bf)   # (4 | m: no tile spans two batches)
    want[p.iA] = Pb
    assert np.array_equal(host_bits(Aout), want), "A_out: pruned region or padding differs"
    got = p.result()
    P = f64_of(Pb, bf).reshape(p.batch, m, k)
    Bm = f64_of(p.b_compact(), bf).reshape(k, n)
    ref = np.stack([P[b] @ Bm for b in range(p.batch)]).reshape(-1)
    scale = np.stack([np.abs(P[b]) @ np.abs(Bm) for b in range(p.batch)]).reshape(-1)
    check_close(f64_of(got, bf), ref, scale, FP16_TOL, f"strided prune24_spmma {shape} {alg} {DT_IDS[bf]}", k, "bf16" if bf else "f16")


# ---------------------------------------------------------------------------------------------
# the staged sm_spmma_{f16,bf16}: one shape per launch class of spmma16() (csrc/spmma_f16.hip), gapped B and C, offset C
# ---------------------------------------------------------------------------------------------
# (per-batch B: the batches are not stacked, so a launch sees m rows x batch = 2; tiles = ceil(m / 128) x ceil(n / 128) x 2:
#  202 rows -> 2 x 2 x 2 = 8; 16386 -> 129 x 2 x 2 = 516; 32770 -> 257 x 2 x 2 = 1028; n <= 64: 65538 -> 513 x 2 = 1026.  The rule reads
#  the shape only -- no CU count -- so the class follows from this table; a moved threshold in spmma16() needs this table moved too.)
STAGED_CLASSES = {   # class -> (m, n, k, layout)
    "pc_256x128": (16402, 136, 1024, dict(gapB=8, gapC=8)),                # 128 <= n <= 256, k >= 1024, >= 16384 rows per launch
    "pc_128x128": (202, 136, 576, dict(gapB=8, gapC=8)),                   # k >= 512, n > 64
    "dma_128x64_w2": (202, 40, 128, dict(gapB=8, gapC=8)),                 # n <= 64, < 1024 tiles
    "dma_128x64_w1": (65538, 40, 64, dict(gapB=8, gapC=8)),                # n <= 64, >= 1024 tiles
    "dma_128x128_w4": (202, 136, 128, dict(gapB=8, gapC=8)),               # < 512 tiles
    "dma_128x128_w2x4": (16386, 136, 64, dict(gapB=8, gapC=8)),            # 512 .. 1023 tiles
    "dma_128x128_w2x2": (32770, 136, 64, dict(gapB=8, gapC=8)),            # >= 1024 tiles
    "cfg_odd_m_64": (201, 40, 128, dict(gapB=8, gapC=8)),
    "cfg_odd_m_128": (201, 136, 128, dict(gapB=8, gapC=8)),
    "cfg_strideB%8": (202, 136, 128, dict(gapB=4, gapC=8)),
    "cfg_B_2byte": (202, 136, 128, dict(gapB=8, gapC=8, offB=1)),
}


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("variant", ["gaps", "sC+3", "c_off1", "ab"])
@pytest.mark.parametrize("cls", list(STAGED_CLASSES))
def test_staged_spmma_on_padded_operands(gpu, orc, cls, variant, bf):
    import torch
    m, n, k, lay = STAGED_CLASSES[cls]
    lay = dict(lay)
    lay.update({"gaps": {}, "sC+3": dict(gapC=3), "c_off1": dict(offC=1), "ab": dict(alpha=0.5, beta=-2.0)}[variant])
    p = Problem(np.random.default_rng(_seed(cls, variant, bf)), m, n, k, Layout(**lay), bf, slack_rows=0)
    blob = torch.empty(gpu.compress24_size(m, k, 2, p.batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dev(p.a_compact(), bf), m, k, k, p.batch, m * k, blob)
    gpu.spmma(blob, p.pB, p.pC, m, n, k, p.batch, p.sB, p.sC, alpha=p.lay.alpha, beta=p.lay.beta)
    p.check(orc, f"strided staged {cls} {variant} {DT_IDS[bf]}")


# ---------------------------------------------------------------------------------------------
# the dense denominator sm_gemm_rowmajor_{f16,bf16}: vector classes x tile shapes (launch_gemm_f16, csrc/gemm_f16.hip)
# ---------------------------------------------------------------------------------------------
VEC_CLASSES = {"vec8": dict(lda_pad=8, gapA=64, offA=0), "vec4": dict(lda_pad=4, gapA=4, offA=4), "vec1": dict(lda_pad=1, gapA=3, offA=1)}
GEMM_TILES = {"N<=64": (200, 40), "M<=64": (40, 104), "other": (200, 104)}


def _run_gemm(gpu, p):
    gpu.gemm_rowmajor(p.pA, p.pB, p.pC, p.m, p.n, p.k, lda=p.lda, batch=p.batch, strideA=p.sA, strideB=p.sB, strideC=p.sC, alpha=p.lay.alpha, beta=p.lay.beta)


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("k", [128, 72], ids=["k128_dma", "k72_cfg"])
@pytest.mark.parametrize("tile", list(GEMM_TILES))
@pytest.mark.parametrize("vec", list(VEC_CLASSES))
def test_gemm_rowmajor_on_padded_operands(gpu, orc, vec, tile, k, bf):
    """vec8 / vec4 / vec1 from lda, strideA and the A base (16-, 8-, 2-byte aligned) x the three tile shapes; whole stages (the
    LDS-DMA kernels where rows are 8-byte aligned) and a ragged k (launch_cfg at that vector width); per-batch B, a C gap."""
    m, n = GEMM_TILES[tile]
    p = Problem(np.random.default_rng(_seed(vec, tile, k, bf)), m, n, k, Layout(gapB=8, gapC=8, **VEC_CLASSES[vec]), bf, dense=True)
    _run_gemm(gpu, p)
    p.check(orc, f"strided gemm {vec} {tile} k={k} {DT_IDS[bf]}")


GEMM_EXTRA = {
    "twin_big": ((240, 200, 2048), dict(lda_pad=8, gapA=64, gapB=8, gapC=8)),        # dense twin, 256 x 256 tiles (128 < n <= 256, k >= 2048)
    "twin_span": ((200, 72, 200), dict(batch=1, offA=8, offB=8, offC=8)),            # dense twin, span form (ragged k, lda == k)
    "ragged_k_padded": ((200, 72, 200), dict(lda_pad=8, gapA=64, gapB=8, gapC=8)),   # ragged k the twin declines (lda != k)
    "alpha_beta": ((200, 104, 128), dict(lda_pad=8, gapA=64, gapB=8, gapC=8, alpha=0.5, beta=-2.0)),
    "alpha_beta_vec1": ((200, 104, 128), dict(lda_pad=1, gapA=3, offA=1, gapB=8, gapC=3, alpha=0.5, beta=-2.0)),
    "c_off1": ((200, 104, 128), dict(lda_pad=8, gapB=8, offC=1)),
    "shared_b_stacked": ((200, 104, 128), dict(lda_pad=8)),
}


@pytest.mark.parametrize("bf", DT, ids=DT_IDS)
@pytest.mark.parametrize("name", list(GEMM_EXTRA))
def test_gemm_rowmajor_routes_on_padded_operands(gpu, orc, name, bf):
    (m, n, k), lay = GEMM_EXTRA[name]
    p = Problem(np.random.default_rng(_seed(name, bf)), m, n, k, Layout(**lay), bf, dense=True)
    _run_gemm(gpu, p)
    p.check(orc, f"strided gemm {name} {DT_IDS[bf]}")


def test_gemm_rowmajor_integer_exact_on_padded_operands(gpu, orc):
    for vec in VEC_CLASSES:
        for bf in DT:
            p = Problem(np.random.default_rng(_seed(vec, "int", bf)), 200, 104, 128, Layout(gapB=8, gapC=8, **VEC_CLASSES[vec]), bf, kind="ties", int_b=True, dense=True)
            _run_gemm(gpu, p)
            p.check(orc, f"strided gemm integer {vec} {DT_IDS[bf]}", exact=True)


# ---------------------------------------------------------------------------------------------
# margins of this file's comparisons, appended to the session's report
# ---------------------------------------------------------------------------------------------
_strided_margin_report = margin_report_fixture(
    "{n} comparisons of tests/test_gpu_strided16.py against the fp64 product; err / (ROUND*|ref| + 2k*ACC*sum|ab| + TINY), worst first:")
