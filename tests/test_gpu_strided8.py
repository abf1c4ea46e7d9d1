"""The 1-byte (fp8 / int8) 2:4 and dense kernels on PADDED operands, per launch class (-m gpu).

Every case places the logical operands in larger buffers (base offsets, lda > k, gaps in the batch strides).  A and B outside the
logical operand hold poison -- the NaN byte of the operand's fp8 format (0x7F e4m3, 0x7E e5m2), 127 for int8 -- and C outside the
logical result holds 0x5A bytes: a kernel that reads padding into a product shows a NaN (or another integer), one that writes outside
its tile changes a sentinel.  The references are NOT the library: the gathered logical A, pruned by the oracle's STRIP rule on the
compact copy (fp8: on its fp16 image), times the gathered B in numpy -- int64 for int8 (exact), fp64 for fp8.  fp8 operands are drawn
from EXACT_VALS with row scales in {0.5, 1, 2} and (alpha, beta) in {(1, 0), (0.5, -2)}, so every fp32 product, sum, scale and add is
exact and C must equal the fp64 result rounded once, bit for bit (the premise is asserted per case: Problem.assert_exact_premise);
random finite operands are held to the dense 1-byte GEMM's bound (b8_testlib's constants) on the layout `all`.  Every fused call must
also equal, bit for bit, prune + compress + the staged matmul on compact copies (include/sparsifyme.h).

The launch classes of launch_spmma_b8 (csrc/spmma_b8.h) are fixed by n alone, so a shape pins the kernel that runs:

    class                                              case (m = 200, k in {64: one plane, 192: odd planes, 256: even planes})
    staged <64,4,1>, fused / dense <64,4,1>            n = 40 (vector store), 37 (per-element), _q: 48 (vector), 40 and 37 (per-element)
    staged <64,4,1>, fused / dense <128,4,2>           n = 104, _q also 112 (vector)
    staged <128,2,4>, fused / dense <128,4,2>          n = 136 (ragged second column tile), _q also 144 (vector)
    both sides of the thresholds                       n = 64 / 68 (fused, dense), 128 / 132 (staged): THRESHOLDS
    folded tall grid                                   lda+16, lda+64, c_off1, off16 and `tall` (batch 3, row_scale[gr % m]); staged: sA+64 too
    per-batch grid (b > 0 with p.sA / row_base)        sA+64, sB+16, sC+8, sC+3, ab, all
    vector store of batch 0, per-element of batch 1    sC+3;  per-element everywhere: c_off1, n = 37
    a non-default lda / ld, a strideA gap              lda+16, lda+64, sA+64, all; PRUNE_CASES (ld), COMPRESS_CASES (ld, strideA)
    a strideB gap, a strideC gap, an unaligned C       sB+16, all; sC+8, sC+3, ab, all; sC+3, c_off1
    odd m                                              test_odd_m_on_padded_operands (dense, sm_spmma_fused_i8), REFUSALS (the others)"""
import numpy as np
import pytest

from b8_testlib import EXACT_VALS, FMTS, OUTS, PAIRS, ROUND, TINY, finite_bytes, img16, ksteps, make_bytes, map_back, odt, ref_quant_rows, tdt, to8, val64
from guard_testlib import Guarded, Layout, Strided, margin_report_fixture, seed
from parity_testlib import MARGINS

pytestmark = pytest.mark.gpu

POISON = {"e4m3": 0x7F, "e5m2": 0x7E, "i8": 0x7F}     # NaN of the format; 127
SENT_BYTE = 0x5A
ELT = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16, "i32": np.uint32, "q": np.uint8}   # C as bit patterns
Q_SCALES = (2.0 ** -8, 0.0123)
UNIT = 0.0625   # the smallest increment of an exact case: products are multiples of 0.25, alpha and row_scale halve it once each


def sentinel(dt):
    return np.frombuffer(bytes([SENT_BYTE] * np.dtype(dt).itemsize), dtype=dt)[0]


def _seed(*xs):
    return seed(0x5718, *xs)


# ---------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------
def c_torch(out):
    import torch
    return {"i32": torch.int32, "q": torch.int8}.get(out) or odt(out)


def bits_of(x, out):
    """fp64 values (exact in fp32) rounded once, to nearest even, to the output type, as bit patterns."""
    import torch
    if out == "f32":
        return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(odt(out))
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def vals_of(b, out):
    import torch
    if out == "f32":
        return b.view(np.float32).astype(np.float64)
    return torch.from_numpy(b.view(np.int16).copy()).view(odt(out)).to(torch.float64).numpy()


def dev_bytes(a, kind):
    """uint8 host bytes -> device tensor of the operand's dtype (fp8 format or int8)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()
    return t.view(torch.int8 if kind == "i8" else tdt(kind))


def dev_c(c, out):
    import torch
    signed = {1: np.int8, 2: np.int16, 4: np.int32}[c.dtype.itemsize]
    return torch.from_numpy(c.view(signed).copy()).cuda().view(c_torch(out))


def host_c(t):
    import torch
    torch.cuda.synchronize()
    it = {1: (torch.int8, np.uint8), 2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32)}[t.element_size()]
    return t.view(it[0]).cpu().numpy().view(it[1])


def host_bytes(t):
    import torch
    torch.cuda.synchronize()
    return t.view(torch.uint8).cpu().numpy()


def prune_strip_ref(orc, a, kind, rows, k, alg=None):
    """The oracle's prune of compact bytes: the int8 rule, or the fp16 rule on the fp8 bytes' exact fp16 image, mapped back."""
    alg = orc.STRIP if alg is None else alg
    if kind == "i8":
        return orc.prune24(np.ascontiguousarray(a, dtype=np.uint8), rows, k, k, alg)
    im = img16(a, kind)
    return map_back(orc.prune24(im, rows, k, k, alg), im, a)


def blob_ref(orc, a, kind, m, k, batch):
    """The blob of compact bytes a ([batch * m][k]), from the oracle alone.  int8: orc.compress24.  fp8: the oracle decides the kept
    positions on the fp16 image (its metadata section is the 1-byte blob's as it is: same geometry); the kept BYTES are gathered
    from a at those positions, and every alignment gap is zero."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if kind == "i8":
        return orc.compress24(a, m, k, k, batch)
    M = m * batch
    kc, mo16, _ = orc.compress24_layout(m, k, 2, batch)
    kc8, mo8, tot8 = orc.compress24_layout(m, k, 1, batch)
    assert kc == kc8
    meta = orc.compress24(img16(a, kind), m, k, k, batch)[mo16: mo16 + M * kc // 8]
    blob = np.zeros(tot8, dtype=np.uint8)
    blob[mo8: mo8 + meta.size] = meta
    nib = np.stack([meta & 0xF, meta >> 4], axis=-1).reshape(kc // 64, M, 16)      # [plane][row][strip]
    Ap = np.zeros((M, kc), dtype=np.uint8)
    Ap[:, :k] = a.reshape(M, k)
    A4 = Ap.reshape(M, kc // 64, 16, 4).transpose(1, 0, 2, 3)                       # [plane][row][strip][4]
    v0 = np.take_along_axis(A4, (nib & 3)[..., None].astype(np.int64), 3)
    v1 = np.take_along_axis(A4, (nib >> 2)[..., None].astype(np.int64), 3)
    vals = np.concatenate([v0, v1], axis=-1).reshape(-1)                            # [plane][row][32 B]
    blob[: vals.size] = vals
    return blob


# ---------------------------------------------------------------------------------------------
# the layout builder
# ---------------------------------------------------------------------------------------------
class Problem(Strided):
    """Padded host buffers, index maps of the logical operands, the references and -- after to_device(), which the constructor calls
    unless told upload=False -- the device copies.  fa / fb: "e4m3", "e5m2" or "i8" (both); out: "f32" / "f16" / "bf16" (fp8), "i32" / "q"
    (int8); data: "exact" or "rand" (fp8).  beta != 0 means accumulate for an int32 C.  (B is stored [n][k]: k * n elements all the same.)"""

    def __init__(self, rng, m, n, k, lay, fa, fb, out, data="exact", slack_rows=64, upload=True):
        Strided.__init__(self, m, n, k, lay, lay.offA, lay.offB, lay.offC)
        self.fa, self.fb, self.out, self.data = fa, fb, out, data
        self.i8 = fa == "i8"
        batch, nb, lda = self.batch, self.nb, self.lda
        # slack after each buffer: whole-tile reads past a ragged m or n stay inside the allocations
        self.gA = Guarded(lay.offA + batch * self.sA + slack_rows * lda + 256, POISON[fa], np.uint8, lay.offA, self.iA)
        self.gB = Guarded(lay.offB + nb * self.sBe + 64 * k + 256, POISON[fb], np.uint8, lay.offB, self.iB)
        self.gC = Guarded(lay.offC + batch * self.sC + 256, sentinel(ELT[out]), ELT[out], lay.offC, self.iC)
        self.A, self.B, self.C = self.gA.host, self.gB.host, self.gC.host
        if self.i8:
            a = rng.integers(-128, 128, (batch * m, k)).astype(np.int8)
            a[:, 0], a[:, -1] = -128, 127
            b = rng.integers(-128, 128, (nb * n, k)).astype(np.int8)
            b[0] = -128
            self.A[self.iA], self.B[self.iB] = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
        elif data == "exact":
            self.A[self.iA] = to8(rng.choice(EXACT_VALS, batch * m * k), fa)
            self.B[self.iB] = to8(rng.choice(EXACT_VALS, nb * n * k), fb)
        else:
            self.A[self.iA] = finite_bytes(rng, batch * m * k, fa)
            self.B[self.iB] = finite_bytes(rng, nb * n * k, fb)
        self.reads_c = lay.beta != 0.0 and out != "q"
        if not self.reads_c:
            self.C0 = np.full(batch * m * n, sentinel(ELT[out]), dtype=ELT[out])
        elif out == "i32":
            self.C0 = rng.integers(-2 ** 20, 2 ** 20, batch * m * n).astype(np.int32).view(np.uint32)
        else:
            self.C0 = bits_of(rng.choice(EXACT_VALS, batch * m * n) if data == "exact" else rng.uniform(-4, 4, batch * m * n), out)
        self.C[self.iC] = self.C0
        # row_scale: m values, then NaN (a kernel that indexed it by the row of the TALL matrix would read them)
        self.rs = None
        if lay.rs and not self.i8:
            self.rs = (rng.choice(np.array([0.5, 1.0, 2.0]), m) if data == "exact" else rng.uniform(0.25, 2.0, m)).astype(np.float32)
        self._refs = {}
        if upload:
            self.to_device()

    def to_device(self):
        import torch
        lay = self.lay
        if self.rs is not None:
            self.drs = torch.from_numpy(np.concatenate([self.rs, np.full(1024, np.nan, dtype=np.float32)])).cuda()
        self.dA = self.gA.to_device().dev.view(torch.int8 if self.i8 else tdt(self.fa))
        self.dB = self.gB.to_device().dev.view(torch.int8 if self.i8 else tdt(self.fb))
        self.dC = self.gC.to_device().dev.view(c_torch(self.out))
        self.pA, self.pB, self.pC = self.dA[lay.offA:], self.dB[lay.offB:], self.dC[lay.offC:]
        return self

    def a_compact(self):
        return self.A[self.iA].copy()

    def b_compact(self):
        return self.B[self.iB].copy()

    def reset_c(self):
        self.dC = self.gC.to_device().dev.view(c_torch(self.out))
        self.pC = self.dC[self.lay.offC:]

    # ---- references -------------------------------------------------------------------------
    def products(self, orc, dense):
        """(A' . B, |A'| . |B|) per batch with A' the oracle's STRIP prune of the compact A (dense: A itself): int64 for int8
        (the second is None), fp64 for fp8."""
        if dense in self._refs:
            return self._refs[dense]
        m, n, k, batch = self.m, self.n, self.k, self.batch
        a = self.a_compact() if dense else prune_strip_ref(orc, self.a_compact(), self.fa, batch * m, k)
        if self.i8:
            A = a.view(np.int8).astype(np.int64).reshape(batch, m, k)
            B = self.b_compact().view(np.int8).astype(np.int64).reshape(self.nb, n, k)
            r = (np.stack([A[b] @ B[b % self.nb].T for b in range(batch)]), None)
        else:
            A, B = val64(a, self.fa).reshape(batch, m, k), val64(self.b_compact(), self.fb).reshape(self.nb, n, k)
            r = (np.stack([A[b] @ B[b % self.nb].T for b in range(batch)]), np.stack([np.abs(A[b]) @ np.abs(B[b % self.nb]).T for b in range(batch)]))
        self._refs[dense] = r
        return r

    def reference(self, orc, dense):
        """(ref, scale) of an fp8 call in fp64: alpha * row_scale[i] * (A' . B) + beta * C0."""
        prod, absprod = self.products(orc, dense)
        s = self.lay.alpha * (self.rs.astype(np.float64)[None, :, None] if self.rs is not None else 1.0)
        c0 = vals_of(self.C0, self.out).reshape(prod.shape) if self.reads_c else 0.0
        return s * prod + self.lay.beta * c0, np.abs(s) * absprod + abs(self.lay.beta) * np.abs(c0)

    def assert_exact_premise(self, orc):
        """Every |result| and sum |a||b| of this case stays below 2^24 units of the smallest increment, so each fp32 product,
        partial sum, scale and add the kernels make is exact."""
        for dense in (False, True):
            ref, scale = self.reference(orc, dense)
            assert np.array_equal(ref, np.round(ref / UNIT) * UNIT), "a result is no multiple of the smallest increment"
            assert max(np.abs(ref).max(), scale.max()) / UNIT < 2.0 ** 24

    # ---- results ----------------------------------------------------------------------------
    def result(self, what):
        """The logical C as bits, after asserting that every sentinel outside it kept its bits."""
        return self.gC.result(lambda n, first: f"{what}: {n} elements of C outside the logical result were written, first at {first}")

    def _where(self, idx):
        return np.unravel_index(idx[:4], (self.batch, self.m, self.n))

    def check_fp8(self, orc, what, dense):
        got = self.result(what)
        g64 = vals_of(got, self.out)
        bad = np.flatnonzero(~np.isfinite(g64))
        assert bad.size == 0, f"{what}: {bad.size} non-finite results (padding read into a product?), first at (batch, row, col) {self._where(bad)}"
        ref, scale = self.reference(orc, dense)
        ref, scale = ref.reshape(-1), scale.reshape(-1)
        if self.data == "exact":
            wrong = np.flatnonzero(got != bits_of(ref, self.out))
            assert wrong.size == 0, f"{what}: {wrong.size} results are not the exact product rounded once, first at (batch, row, col) {self._where(wrong)}"
        else:   # the dense 1-byte GEMM's bound, from b8_testlib's constants
            bound = ROUND[self.out] * np.abs(ref) + (2.0 * ksteps(self.k) + 4.0) * 2.0 ** -24 * scale + TINY[self.out]
            ratio = float((np.abs(g64 - ref) / bound).max())
            print(f"{what}: err/bound {ratio:.3f}")
            MARGINS.append((what, ratio))
            assert ratio <= 1.0, f"{what}: err/bound {ratio:.3f} (m, n, k) = {(self.m, self.n, self.k)}, ksteps {ksteps(self.k)}"
        return got

    def check_i8(self, orc, what, dense, scale=None):
        got = self.result(what)
        acc, _ = self.products(orc, dense)
        if self.out == "q":
            want = orc.requant_i8(np.ascontiguousarray(acc.reshape(-1).astype(np.int32)), scale).view(np.uint8)
        else:
            want = acc.reshape(-1) + (self.C0.view(np.int32).astype(np.int64) if self.reads_c else 0)
            want = want.astype(np.int32).view(np.uint32)
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, f"{what}: {wrong.size} results differ from the integer product, first at (batch, row, col) {self._where(wrong)}"
        return got

    def check(self, orc, what, dense=False, scale=None):
        return self.check_i8(orc, what, dense, scale) if self.i8 else self.check_fp8(orc, what, dense)

    # ---- calls ------------------------------------------------------------------------------
    def _kw(self, scale=None):
        lay = self.lay
        if self.i8:
            return dict(scale=scale) if self.out == "q" else dict(accumulate=self.reads_c)
        return dict(alpha=lay.alpha, beta=lay.beta, row_scale=None if self.rs is None else self.drs)

    def run_fused(self, gpu, scale=None, **over):
        kw = dict(lda=self.lda, batch=self.batch, strideA=self.sA, strideB=self.sB, strideC=self.sC)
        kw.update(self._kw(scale))
        kw.update(over)
        (gpu.spmma_fused_i8 if self.i8 else gpu.spmma_fused_fp8)(self.pA, self.pB, self.pC, self.m, self.n, self.k, **kw)

    def run_dense(self, gpu, scale=None, **over):
        kw = dict(lda=self.lda, batch=self.batch, strideA=self.sA, strideB=self.sB, strideC=self.sC)
        kw.update(self._kw(scale))
        kw.update(over)
        if not self.i8:
            gpu.gemm_rowmajor_fp8(self.pA, self.pB, self.pC, self.m, self.n, self.k, **kw)
        elif self.out == "q":
            gpu.gemm_rowmajor_i8_q(self.pA, self.pB, self.pC, self.m, self.n, self.k, kw.pop("scale"), **kw)
        else:
            gpu.gemm_rowmajor_i8(self.pA, self.pB, self.pC, self.m, self.n, self.k, **kw)

    def _staged(self, gpu, blob, B, C, sB, sC, scale, **over):
        m, n, k = self.m, self.n, self.k
        args = dict(batch=self.batch, strideB=sB, strideC=sC)
        args.update(over)
        if not self.i8:
            gpu.spmma_fp8(blob, B, C, m, n, k, a_dtype=tdt(self.fa), **args, **self._kw())
        elif self.out == "q":
            gpu.spmma_i8_q(blob, B, C, m, n, k, scale, **args)
        else:
            gpu.spmma_i8(blob, B, C, m, n, k, accumulate=self.reads_c, **args)

    def compress_padded(self, gpu, orc):
        """The blob of the PADDED A (ld = lda, strideA with its gap, the base offset), held against the oracle's blob of the
        compact copy -- gaps included -- before any matmul reads it."""
        import torch
        m, k, batch = self.m, self.k, self.batch
        blob = torch.full((gpu.compress24_size(m, k, 1, batch),), 0xAB, dtype=torch.uint8, device="cuda")
        (gpu.compress24 if self.i8 else gpu.compress24_fp8)(self.pA, m, k, self.lda, batch, self.sA, blob)
        want = blob_ref(orc, self.a_compact(), self.fa, m, k, batch)
        assert np.array_equal(host_bytes(blob), want), "the blob of the padded A differs from the oracle's blob of the compact copy"
        return blob

    def run_staged(self, gpu, blob, scale=None, **over):
        self._staged(gpu, blob, self.pB, self.pC, self.sB, self.sC, scale, **over)

    def contract_bits(self, gpu, scale=None):
        """prune + compress + the staged matmul on COMPACT copies of the same operands: the bits a fused call must return."""
        import torch
        m, n, k, batch = self.m, self.n, self.k, self.batch
        tail = np.full(256, sentinel(ELT[self.out]), dtype=ELT[self.out])      # sentinels after the compact C as well
        dAc, dBc, dCc = dev_bytes(self.a_compact(), self.fa), dev_bytes(self.b_compact(), self.fb), dev_c(np.concatenate([self.C0, tail]), self.out)
        (gpu.prune24 if self.i8 else gpu.prune24_fp8)(dAc, dAc, batch * m, k, k, gpu.PRUNE_STRIP)
        blob = torch.empty(gpu.compress24_size(m, k, 1, batch), dtype=torch.uint8, device="cuda")
        (gpu.compress24 if self.i8 else gpu.compress24_fp8)(dAc, m, k, k, batch, m * k, blob)
        self._staged(gpu, blob, dBc, dCc, 0 if self.nb == 1 else n * k, m * n, scale)
        got = host_c(dCc)
        assert np.array_equal(got[self.C0.size:], tail), "the staged matmul on compact copies wrote past the end of C"
        return got[: self.C0.size]


def run_entries(gpu, orc, p, what, fused=True, dense=True, staged=True):
    """Every entry point of p's family on p's layout: the fused form (also against the staged pair on compact copies), the dense
    GEMM, and compress of the padded A + the staged matmul."""
    if not p.i8 and p.data == "exact":
        p.assert_exact_premise(orc)
    for scale in (Q_SCALES if p.out == "q" else (None,)):
        tag = f"{what}" + (f" scale {scale}" if scale else "")
        if fused:
            p.run_fused(gpu, scale)
            got = p.check(orc, "fused " + tag, scale=scale)
            if p.m % 2 == 0:
                assert np.array_equal(got, p.contract_bits(gpu, scale)), f"fused {tag}: differs from prune + compress + the staged matmul on compact copies"
            p.reset_c()
        if dense:
            p.run_dense(gpu, scale)
            p.check(orc, "dense " + tag, dense=True, scale=scale)
            p.reset_c()
        if staged:
            blob = p.compress_padded(gpu, orc)
            p.run_staged(gpu, blob, scale)
            p.check(orc, "staged " + tag, scale=scale)
            p.reset_c()


# ---------------------------------------------------------------------------------------------
# matmul: launch class x layout
# ---------------------------------------------------------------------------------------------
M = 200
KS = (64, 192, 256)          # one plane (the tail is the first stage); odd plane count; even plane count
NS = {"fp8": (40, 104, 136, 37), "i32": (40, 104, 136, 37), "q": (48, 104, 136, 40, 37, 112, 144)}
LAYOUTS = {
    "lda+16": dict(lda_pad=16),
    "lda+64": dict(lda_pad=64),
    "sA+64": dict(gapA=64),                      # un-folds the tall matrix of fused and dense: shared B on the per-batch grid
    "sB+16": dict(gapB=16),                      # per-batch B with a gap
    "sC+8": dict(gapC=8, rs=True),               # un-folds the staged path with shared B: row_base and row_scale[gr] on b > 0
    "sC+3": dict(gapC=3, rs=True),               # batch 1's C leaves the vector-store alignment, batch 0 keeps it
    "c_off1": dict(offC=1),
    "off16": dict(offA=16, offB=16),
    "tall": dict(batch=3, rs=True),              # contiguous: one tall matrix, a row tile straddles two batches (200 rows, BM = 128)
    "ab": dict(gapC=8, alpha=0.5, beta=-2.0, rs=True),      # int32: accumulate
    "all": dict(lda_pad=16, gapA=64, gapB=16, gapC=8, offA=16, offB=16, alpha=0.5, beta=-2.0, rs=True),
}
FAMILY = {"fp8": ("e4m3", "e5m2", "f32"), "i32": ("i8", "i8", "i32"), "q": ("i8", "i8", "q")}
# every (n, k) on `all` (per-batch grid) and `tall` (folded); the other layouts walk the k's per n
CASES = [(fam, lname, n, k) for fam in NS for lname in ("all", "tall") for n in NS[fam] for k in KS]
CASES += [(fam, lname, n, KS[(i + j) % 3]) for fam in NS for i, lname in enumerate(LAYOUTS) if lname not in ("all", "tall") for j, n in enumerate(NS[fam])]


def _cid(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_matmul_on_padded_operands(gpu, orc, case):
    fam, lname, n, k = case
    fa, fb, out = FAMILY[fam]
    p = Problem(np.random.default_rng(_seed(*case)), M, n, k, Layout(**LAYOUTS[lname]), fa, fb, out)
    run_entries(gpu, orc, p, _cid(case))


@pytest.mark.parametrize("lname", ["all", "sC+3"])
@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("fa,fb", PAIRS)
def test_fp8_formats_and_outputs_on_padded_operands(gpu, orc, fa, fb, out, lname):
    """All four format pairs and all three output types, one (n, k) per launch class."""
    for j, n in enumerate(NS["fp8"]):
        k = KS[(j + FMTS.index(fa) + OUTS.index(out)) % 3]
        p = Problem(np.random.default_rng(_seed(fa, fb, out, lname, n)), M, n, k, Layout(**LAYOUTS[lname]), fa, fb, out)
        run_entries(gpu, orc, p, f"{fa}x{fb}->{out} {lname} n={n} k={k}")


THRESHOLDS = (64, 68, 128, 132)   # fused / dense: BN 64 up to n = 64; staged: BN 64 up to n = 128


@pytest.mark.parametrize("n", THRESHOLDS)
@pytest.mark.parametrize("fam", list(FAMILY))
def test_both_sides_of_each_threshold(gpu, orc, fam, n):
    fa, fb, out = FAMILY[fam]
    p = Problem(np.random.default_rng(_seed(fam, "thr", n)), M, n, 192, Layout(**LAYOUTS["all"]), fa, fb, out)
    run_entries(gpu, orc, p, f"{fam} threshold n={n}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS["fp8"])
def test_fp8_random_operands_within_the_dense8_bound(gpu, orc, n, k):
    """Random finite operands on the layout `all`, per entry point and class: the dense 1-byte GEMM's bound, ratios to the margins report."""
    out = OUTS[(NS["fp8"].index(n) + KS.index(k)) % 3]
    p = Problem(np.random.default_rng(_seed("rand", n, k)), M, n, k, Layout(**LAYOUTS["all"]), "e4m3", "e5m2", out, data="rand")
    run_entries(gpu, orc, p, f"strided8 random e4m3xe5m2->{out} all (m, n, k) = {(M, n, k)}")


# the entry points that take any m: the dense GEMMs and sm_spmma_fused_i8[_q]
@pytest.mark.parametrize("lname", ["all", "tall"])
@pytest.mark.parametrize("n", [40, 136])
@pytest.mark.parametrize("fam", list(FAMILY))
def test_odd_m_on_padded_operands(gpu, orc, fam, n, lname):
    import torch
    fa, fb, out = FAMILY[fam]
    m, k = 201, 192
    p = Problem(np.random.default_rng(_seed(fam, "odd", n, lname)), m, n, k, Layout(**LAYOUTS[lname]), fa, fb, out)
    run_entries(gpu, orc, p, f"{fam} m=201 n={n} {lname}", fused=p.i8, staged=False)
    if fam != "i32":
        return
    # sm_spmma_fused_i8 at an odd m equals sm_gemm_rowmajor_i8 of the STRIP-pruned compact A
    p.run_fused(gpu)
    got = p.result("fused i8 m=201")
    pruned = dev_bytes(prune_strip_ref(orc, p.a_compact(), "i8", p.batch * m, k), "i8")
    Cd = dev_c(p.C0.copy(), "i32")
    gpu.gemm_rowmajor_i8(pruned, dev_bytes(p.b_compact(), "i8"), Cd, m, n, k, batch=p.batch, strideB=0 if p.nb == 1 else n * k, accumulate=p.reads_c)
    assert np.array_equal(got, host_c(Cd))


# ---------------------------------------------------------------------------------------------
# refusals: decided before any device work, C untouched
# ---------------------------------------------------------------------------------------------
# name -> (layout, overrides of the call, m, k, status, which entries: f = fused, d = dense, s = staged)
REFUSALS = {
    "lda%16": (dict(lda_pad=8), {}, 200, 192, 2, "fd"),
    "strideA%16": (dict(gapA=8), {}, 200, 192, 2, "fd"),
    "strideB%16": (dict(gapB=8), {}, 200, 192, 2, "fds"),
    "A_base+8": (dict(offA=8), {}, 200, 192, 2, "fd"),
    "B_base+8": (dict(offB=8), {}, 200, 192, 2, "fds"),
    "k=96": (dict(), {}, 200, 96, 2, "fds"),
    "lda<k": (dict(), dict(lda=176), 200, 192, 1, "fd"),
    "odd_m": (dict(), {}, 201, 192, 2, "Fs"),     # F: the fp8 fused form only (sm_spmma_fused_i8 takes an odd m)
}


@pytest.mark.parametrize("fam", list(FAMILY))
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_c_alone(gpu, orc, name, fam):
    import torch
    lay, over, m, k, status, entries = REFUSALS[name]
    fa, fb, out = FAMILY[fam]
    p = Problem(np.random.default_rng(_seed(name, fam)), m, 40, k, Layout(**lay), fa, fb, out)
    scale = Q_SCALES[0] if out == "q" else None
    blob = torch.zeros(gpu.compress24_size(m + 1, k, 1, p.batch), dtype=torch.uint8, device="cuda")
    calls = []
    if "f" in entries or ("F" in entries and not p.i8):
        calls.append(lambda: p.run_fused(gpu, scale, **over))
    if "d" in entries:
        calls.append(lambda: p.run_dense(gpu, scale, **over))
    if "s" in entries:
        calls.append(lambda: p.run_staged(gpu, blob, scale))
    assert calls or name == "odd_m"
    for call in calls:
        with pytest.raises(gpu.SparsifymeError, match=f"status {status}"):
            call()
        assert np.array_equal(host_c(p.dC), p.C), "a refused call wrote to C"


def test_null_operands_are_invalid_values(gpu):
    """A null A (blob), through the C ABI itself: SM_STATUS_INVALID_VALUE whatever else holds."""
    import torch
    L, INV = gpu.lib(), gpu.STATUS_INVALID_VALUE
    z = torch.full((4096,), SENT_BYTE, dtype=torch.uint8, device="cuda")
    B, C, m, n, k = z.data_ptr(), z.data_ptr(), 8, 8, 64
    assert L.sm_spmma_fused_fp8(None, B, C, m, n, k, k, 1, m * k, 0, m * n, 0, 0, 0, 1.0, 0.0, None, None) == INV
    assert L.sm_gemm_rowmajor_fp8(None, B, C, m, n, k, k, 1, m * k, 0, m * n, 0, 0, 0, 1.0, 0.0, None, None) == INV
    assert L.sm_spmma_fp8(None, B, C, m, n, k, 1, 0, m * n, 0, 0, 0, 1.0, 0.0, None, None) == INV
    assert L.sm_spmma_fused_i8(None, B, C, m, n, k, k, 1, m * k, 0, m * n, 0, None) == INV
    assert L.sm_spmma_fused_i8_q(None, B, C, m, n, k, k, 1, m * k, 0, m * n, 1.0, None) == INV
    assert L.sm_gemm_rowmajor_i8(None, B, C, m, n, k, k, 1, m * k, 0, m * n, 0, None) == INV
    assert L.sm_gemm_rowmajor_i8_q(None, B, C, m, n, k, k, 1, m * k, 0, m * n, 1.0, None) == INV
    assert L.sm_spmma_i8(None, B, C, m, n, k, 1, 0, m * n, 0, None) == INV
    assert L.sm_spmma_i8_q(None, B, C, m, n, k, 1, 0, m * n, 1.0, None) == INV
    torch.cuda.synchronize()
    assert bool((z == SENT_BYTE).all())


# ---------------------------------------------------------------------------------------------
# prune / check / compress / decompress with ld > k
# ---------------------------------------------------------------------------------------------
KINDS = ["i8"] + FMTS
DATA = ["rand", "ties", "specials"]


def make_elems(rng, size, kind, data):
    if kind != "i8":
        return make_bytes(rng, size, kind, "special" if data == "specials" else data)
    if data == "rand":
        return rng.integers(-128, 128, size).astype(np.int8).view(np.uint8)
    vals = [-2, -1, 0, 1, 2] if data == "ties" else [-128, 127, -127, 0, 0, -1, 1, 64, -64]
    return rng.choice(np.array(vals, dtype=np.int8), size).view(np.uint8)


def lds_of(k):
    r = (k + 15) // 16 * 16
    return {"r16": r, "r16+16": r + 16, "k+3": k + 3}


class Padded:
    """batch matrices of m x k bytes at `off` in a poison-filled buffer (ld, strideA), and a same-shaped destination of sentinels."""

    def __init__(self, rng, kind, data, m, k, ld, off=0, batch=1, gapA=0):
        self.kind, self.m, self.k, self.ld, self.off, self.batch = kind, m, k, ld, off, batch
        self.sA = m * ld + gapA
        size = off + batch * self.sA + 64
        self.idx = (off + np.arange(batch)[:, None, None] * self.sA + np.arange(m)[None, :, None] * ld + np.arange(k)[None, None, :]).reshape(-1)
        self.src = np.full(size, POISON[kind], dtype=np.uint8)
        self.compact = make_elems(rng, batch * m * k, kind, data)
        self.src[self.idx] = self.compact
        self.sent = np.full(size, SENT_BYTE, dtype=np.uint8)

    def dev(self, a):
        t = dev_bytes(a, self.kind)
        assert t.data_ptr() % 16 == 0
        return t, t[self.off:]

    def expect(self, base, logical):
        want = base.copy()
        want[self.idx] = logical
        return want


PRUNE_CASES = [(kind, m, k, ldn, 0) for kind in KINDS for m in (7, 130) for k in (64, 100, 147) for ldn in ("r16", "r16+16", "k+3")]
PRUNE_CASES += [(kind, 130, 147, "r16", 1) for kind in KINDS]   # the base moved by one byte: every class scalar


@pytest.mark.parametrize("case", PRUNE_CASES, ids=_cid)
def test_prune24_b8_on_padded_rows(gpu, orc, case):
    """STRIP and TILE, in place and out of place: the logical part is the oracle's prune of the compact copy, the padding keeps its
    poison (in place) or the destination's sentinels; with k = 147 / 100 the last strip and tile sit next to poison that must be
    neither selected nor zeroed."""
    kind, m, k, ldn, off = case
    ld = lds_of(k)[ldn]
    prune = gpu.prune24 if kind == "i8" else gpu.prune24_fp8
    for data in DATA:
        P = Padded(np.random.default_rng(_seed(*case, data)), kind, data, m, k, ld, off)
        for alg, oalg in ((gpu.PRUNE_STRIP, orc.STRIP), (gpu.PRUNE_TILE, orc.TILE)):
            want = prune_strip_ref(orc, P.compact, kind, m, k, oalg)
            _, src = P.dev(P.src)
            dst_all, dst = P.dev(P.sent)
            prune(src, dst, m, k, ld, alg)
            assert np.array_equal(host_bytes(dst_all), P.expect(P.sent, want)), f"{case} {data} alg {alg}: out of place"
            in_all, inp = P.dev(P.src)
            prune(inp, inp, m, k, ld, alg)
            assert np.array_equal(host_bytes(in_all), P.expect(P.src, want)), f"{case} {data} alg {alg}: in place"


@pytest.mark.parametrize("case", PRUNE_CASES, ids=_cid)
def test_prune24_check_b8_ignores_the_padding(gpu, orc, case):
    import torch
    kind, m, k, ldn, off = case
    ld = lds_of(k)[ldn]
    check = gpu.prune24_check if kind == "i8" else gpu.prune24_check_fp8
    P = Padded(np.random.default_rng(_seed(*case, "chk")), kind, "rand", m, k, ld, off)
    a = P.expect(P.src, prune_strip_ref(orc, P.compact, kind, m, k))
    a2 = a.reshape(-1)[off: off + m * ld].reshape(m, ld)       # (a view: the rows of the padded matrix)
    a2[:, k:] = 0
    a2[:, k: min(k + 4, ld)] = 0x31                            # a whole non-zero strip, in the padding right after column k only
    valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    check(P.dev(a)[1], m, k, ld, valid)
    assert int(valid.item()) == 0, "non-zeros in the padding were counted"
    a2[m - 1, (k - 1) // 4 * 4: k] = 0x31                      # the last logical strip of the last row: 4 (ragged k: 3) non-zeros
    check(P.dev(a)[1], m, k, ld, valid)
    assert int(valid.item()) == 1, "too many non-zeros in the last logical strip were not seen"


COMPRESS_CASES = [(kind, m, k, ldn, gapA) for kind in KINDS for m in (7, 130) for k in (64, 100, 147) for ldn in ("r16+16", "k+3") for gapA in (32, 0)]
COMPRESS_CASES += [(kind, 130, 147, "r16", 32) for kind in KINDS]


@pytest.mark.parametrize("case", COMPRESS_CASES, ids=_cid)
def test_compress24_decompress24_b8_on_padded_batches(gpu, orc, case):
    """batch 3, ld > k; strideA = m * ld + 32 (the per-item batch division) or m * ld (folds to one tall matrix): the whole blob, its
    zeroed gaps included, is the oracle's blob of the compact copy; decompress into a sentinel-filled padded destination writes the
    oracle's STRIP prune and nothing else."""
    import torch
    kind, m, k, ldn, gapA = case
    ld, batch = lds_of(k)[ldn], 3
    comp, decomp = (gpu.compress24, gpu.decompress24) if kind == "i8" else (gpu.compress24_fp8, gpu.decompress24_fp8)
    for data in DATA:
        P = Padded(np.random.default_rng(_seed(*case, data)), kind, data, m, k, ld, 0, batch, gapA)
        blob = torch.full((gpu.compress24_size(m, k, 1, batch),), 0xAB, dtype=torch.uint8, device="cuda")
        comp(P.dev(P.src)[1], m, k, ld, batch, P.sA, blob)
        assert np.array_equal(host_bytes(blob), blob_ref(orc, P.compact, kind, m, k, batch)), f"{case} {data}: blob"
        dst_all, dst = P.dev(P.sent)
        decomp(blob, m, k, ld, batch, P.sA, dst)
        want = prune_strip_ref(orc, P.compact, kind, batch * m, k)
        assert np.array_equal(host_bytes(dst_all), P.expect(P.sent, want)), f"{case} {data}: decompress"


@pytest.mark.parametrize("src", ["f16", "bf16"])
def test_quantize_compress24_fp8_from_padded_a_drives_spmma_fp8(gpu, orc, src):
    """The two halves joined: sm_quantize_compress24_fp8_* from a 16-bit A with lda > k (NaN in its padding), its blob through
    sm_spmma_fp8 with a strideC gap.  Rows hold {0, +-0.5, +-1, +-2, +-4} x 2^(i % 3) with a +-4 in each, so the quantised bytes are
    exact multiples and row i of every batch has the scale of row i: C = fl32(row_scale[i] * acc) with acc exact."""
    import torch
    m, n, k, batch, lda, gapC, f = 200, 40, 192, 2, 200, 8, "e4m3"
    rng = np.random.default_rng(_seed("quant", src))
    x = rng.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0], dtype=np.float32), (batch * m, k))
    x[:, 5] = 4.0
    x *= (2.0 ** (np.arange(batch * m) % m % 3))[:, None].astype(np.float32)
    a16 = torch.full((batch * m, lda), float("nan"), dtype=odt(src))
    a16[:, :k] = torch.from_numpy(x).to(odt(src))
    q, rs = ref_quant_rows(x, f)
    assert np.array_equal(rs[:m], rs[m:])
    assert gpu.compress24_size(batch * m, k, 1, 1) == gpu.compress24_size(m, k, 1, batch)
    blob = torch.full((gpu.compress24_size(m, k, 1, batch),), 0xAB, dtype=torch.uint8, device="cuda")
    drs = torch.full((batch * m,), -1.0, dtype=torch.float32, device="cuda")
    gpu.quantize_compress24_fp8(a16.cuda(), blob, drs, batch * m, k, tdt(f), lda=lda)
    assert np.array_equal(drs.cpu().numpy().view(np.uint32), rs.view(np.uint32))
    assert np.array_equal(host_bytes(blob), blob_ref(orc, q.reshape(-1), f, m, k, batch))
    p = Problem(rng, m, n, k, Layout(gapC=gapC), f, "e5m2", "f32")
    p.A[p.iA] = q.reshape(-1)      # (the logical A of the reference: the quantised bytes)
    p.drs = torch.from_numpy(np.concatenate([rs[:m], np.full(1024, np.nan, dtype=np.float32)])).cuda()
    gpu.spmma_fp8(blob, p.pB, p.pC, m, n, k, batch=batch, strideB=0, strideC=p.sC, row_scale=p.drs, a_dtype=tdt(f))
    acc, absacc = p.products(orc, False)
    assert absacc.max() < 2.0 ** 24 and np.array_equal(acc, np.round(acc))
    want = (rs[:m].astype(np.float32)[None, :, None] * acc.astype(np.float32)).astype(np.float32)
    assert np.array_equal(p.result("quantised blob through sm_spmma_fp8"), want.reshape(-1).view(np.uint32))


# ---------------------------------------------------------------------------------------------
# margins of this file's random comparisons, appended to the session's report
# ---------------------------------------------------------------------------------------------
_strided8_margin_report = margin_report_fixture(
    "{n} comparisons of tests/test_gpu_strided8.py against the fp64 product; err / (ROUND*|ref| + (2*ksteps(k)+4)*2^-24*sum|ab| + TINY), worst first:")
