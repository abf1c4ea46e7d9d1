"""The pointer-array batched GEMMs (include/sparsifyme.h, a5) per launch class, on guarded operands (-m gpu).

sm_gemm_batched_f16 / _f16_ws / _f32 / _f64 take COLUMN-major operands (lda = m, ldb = k, ldc = m) as device arrays of pointers.  Every
case places each operand family (A, B, C) in a pool: one buffer -- or two, the `second` layouts -- with a 256-byte guard at both ends and
an unequal gap behind every matrix; the matrices sit at NON-MONOTONIC offsets (no stride describes the table), one shared B is the same
pointer repeated (the reference's call), `dupA` makes two entries name the same A.  A and B outside the logical matrices (the guards,
the gaps and -- transposed operands -- the part of a stored row the leading dimension skips) hold a quiet NaN of the type, C outside holds
a sentinel (a NaN too, and with beta == 0 the whole of C does: beta == 0 must not read C).  After every call every guard and gap word of C
is unchanged, A and B come back bit for bit, and the C entries are compared one by one.  Bases stay inside the header's precondition:
f16 / f32 bases at multiples of 16 bytes that are no multiples of 256, f64 bases 16-byte aligned or (`odd8`) at 8 mod 16.

The references are NOT the library: the gathered logical operands multiplied in numpy, fp64 for f16 / f32 and np.longdouble for f64, alpha
and beta applied there.  Two data kinds per case: `ties` (integers in [-3, 3], {-1, 0, 1} from k = 257 on; (alpha, beta) in {(1, 0),
(0.5, -2)}: the result must equal the reference converted to the output type bit for bit, the premise -- the reference is a value of
the output type -- is asserted per case) and `uniform` (U(-1, 1): check_close at FP16_TOL / FP32_TOL / 1e-12 and its ROUND / ACC bound).

Launch classes, in the call's own (m, n, k, batch, ta, tb); the row-major view the kernels see is M = n, N = m, K = k, lda = k, ldb = ldc = m:

    entry   class (CLASS_NEEDS key)      dispatch                          cases
    f64     f64 dma<64,64>               gemm_f32.hip:948                  m in {2, 66, 130} x n in {40, 64, 65, 200}, k in {16, 32, 48}; odd8
    f64     f64 dma<128,128>             gemm_f32.hip:946-947              m = n = 200, k in {16, 48}, batch from the CU count: test_f64_big_tiles
    f64     f64 fma                      gemm_f32.hip:950-951              k = 5, 24; odd m (also at k = 16); the three transposed pairs
    f32     f32 dma<64,64>               gemm_f32.hip:583                  n = 40, m = 40
    f32     f32 dma<64,128>              gemm_f32.hip:583                  n = 40, m = 72 and 200
    f32     f32 dma<128,64>              gemm_f32.hip:584                  n = 200, m = 40 and 104
    f32     f32 dma<128,128>             gemm_f32.hip:584                  n = 200, m = 136
    f32     f32 generic<64,64>           gemm_f32.hip:589                  k = 72, m = 37; k = 5; k = 64 with m = 37
    f32     f32 generic<128,64>          gemm_f32.hip:589                  n = 130, m = 5, k = 40, batch from the CU count: test_f32_generic_128x64
    f32     f32 T dma<64,64>, f32 T dma<64,128>, f32 T dma<128,64>, f32 T dma<128,128>   gemm_f32.hip:876, 583-584 (MODE 2, BKM)   ta = T: the same tilings
    f32     f32 T generic<64,64>         gemm_f32.hip:876, 589             ta = T: k = 72; k = 32 with m = 37
    f32     f32 atr<0>                   gemm_f32.hip:875                  tb = T: m = 131, n = 70, k = 77
    f32     f32 atr<2>                   gemm_f32.hip:874                  ta = tb = T: the same shape
    f16     twin span<64>                spmma_f16_fused.hip:1851          m = 40, k in {72, 147}, n = 200, batch in {3, 11} (11 > MAXG = 8)
    f16     twin span<128>               spmma_f16_fused.hip:1851          m = 104, the same
    f16     twin big<256>                spmma_f16_fused.hip:1871          m in {136, 256}, n = 250, k = 2048, batch 2
    f16_ws  twin streamk                 spmma_f16_fused.hip:1857-1861     the same shapes with a workspace, where sk_takes says so (256 CUs: batch <= 42)
    f16_ws  ws twin big<256>             spmma_f16_fused.hip:1857, 1871    ... and where it does not (batch 43, 44); workspace None / too small: test_ws_entry_without_...
    f16     dma<128,64>                  gemm_f16.hip:528                  m = 40 (m % 8 == 0: the twin declines) and 36 (m % 8 == 4)
    f16     dma<64,128>                  gemm_f16.hip:529                  m = 104 and 132, n = 40
    f16     dma<128,128>                 gemm_f16.hip:530                  m = 104, 132 and 136, n = 200
    f16     cfg<128,64> vec8             gemm_f16.hip:532, 493             m = 40, k = 440: the span form's LDS bound declines
    f16     cfg<64,128> vec8, cfg<128,128> vec8   gemm_f16.hip:533-534, 493   m = 136 (> 128: no span form), k = 72
    f16     cfg<128,64> vec4, cfg<64,128> vec4, cfg<128,128> vec4   gemm_f16.hip:532-534, 494   m % 8 == 4, k = 72; m = 40, k = 76 with odd n
    f16     cfg<128,64> vec1, cfg<64,128> vec1, cfg<128,128> vec1   gemm_f16.hip:532-534, 495   odd m or odd k
    f16     cfg<128,128,T> vec8          gemm_f16.hip:509-511, 493         (T,N), (N,T), (T,T): m = 136, k = 72, n = 40
    f16     cfg<128,128,T> vec4->1       gemm_f16.hip:509-511, 495         a vec 4 request (k % 8 == 4 or m % 8 == 4) runs the vec 1 kernel
    f16     cfg<128,128,T> vec1          gemm_f16.hip:509-511, 495         m = 131, k = 77, n = 35

Every (tile, vec) pair of the register-staged kernel is reachable from this entry point (test_gemm_batched_cases.py enumerates them).
Once per entry point: a NaN in one A reaches exactly the C columns of the entries that name it; batch = 1; a graph captured once on a side
stream (a chain, no parallel branches) whose pointer tables are rewritten in device memory between replays.  Refusals: REFUSALS, called
without a device by test_gemm_batched_cases.py."""
import collections

import numpy as np
import pytest

from guard_testlib import margin_report_fixture, seed
from parity_testlib import FP16_TOL, FP32_TOL, bits, check_close

pytestmark = pytest.mark.gpu


def _seed(*xs):
    return seed(0x5718, *xs)


assert np.finfo(np.longdouble).nmant >= 63, "the f64 reference needs a wider type than the kernel's"

OP_N, OP_T = 0, 1
INVALID, NOT_SUPPORTED = 1, 2
KINDS = ("ties", "uniform")
ABS = ((1.0, 0.0), (0.5, -2.0))
GUARD_BYTES = 256              # in front of and behind every buffer
CAP_BYTES = 64 << 20           # of one case's buffers
MAXG = 8                       # spmma_f16_fused.hip: problems per launch of the grouped entry points (the span twin takes more)
ENTRIES = ("f16", "f16_ws", "f32", "f64")
DT = {"f16": dict(np=np.float16, u=np.uint16, qnan=0x7E00, sent=0x7E5A, wide=np.float64, tol=FP16_TOL),
      "f32": dict(np=np.float32, u=np.uint32, qnan=0x7FC00000, sent=0x7FC5A5A5, wide=np.float64, tol=FP32_TOL),
      "f64": dict(np=np.float64, u=np.uint64, qnan=0x7FF8000000000000, sent=0x7FF85A5A5A5A5A5A, wide=np.longdouble, tol=1e-12)}


def sfx_of(entry):
    return entry[:3]


# ---------------------------------------------------------------------------------------------
# operand placement
# ---------------------------------------------------------------------------------------------
class Pool:
    """`nmat` matrices of `extent` elements in one buffer (or two: `second` moves every third matrix, from matrix 1 on, to a second
    allocation), each buffer filled with `fill`.  base[i]: element offset of matrix i inside buffer alloc[i]."""

    def __init__(self, sfx, extent, nmat, fill, second=False, odd8=False):
        self.u = DT[sfx]["u"]
        self.es = es = np.dtype(self.u).itemsize
        self.extent, self.nmat, self.fill = extent, nmat, self.u(fill)
        q = 16 // es
        assert not odd8 or es == 8
        self.alloc = [1 if second and i % 3 == 1 else 0 for i in range(nmat)]
        self.base = [0] * nmat
        self.buf = []
        for a in (0, 1):
            mats = [i for i in range(nmat) if self.alloc[i] == a]
            order = mats[1::2][::-1] + mats[0::2]            # where the matrices lie, front to back
            cur = GUARD_BYTES // es
            for s, i in enumerate(order):
                b = -(-cur // q) * q
                if (b * es) % 256 == 0:
                    b += q
                self.base[i] = b + (1 if odd8 else 0)
                cur = self.base[i] + extent + q * (1 + (s * s + i) % 5)
            self.buf.append(np.full(cur + GUARD_BYTES // es if mats else 0, self.fill, dtype=self.u))
        self.logical = [np.zeros(b.size, dtype=bool) for b in self.buf]
        self.dbuf = None

    def scatter(self, i, idx, values):
        at = self.base[i] + idx.reshape(-1)
        self.buf[self.alloc[i]][at] = values.reshape(-1)
        self.logical[self.alloc[i]][at] = True

    def gather(self, i, idx, bufs=None):
        return (self.buf if bufs is None else bufs)[self.alloc[i]][self.base[i] + idx.reshape(-1)].reshape(idx.shape)

    def nbytes(self):
        return sum(b.nbytes for b in self.buf)

    def to_device(self):
        import torch
        self.dbuf = [torch.from_numpy(b.view({2: np.int16, 4: np.int32, 8: np.int64}[self.es])).cuda() if b.size else None for b in self.buf]
        for t in self.dbuf:
            assert t is None or t.data_ptr() % 256 == 0      # so that a base's alignment is its offset's
        return self

    def ptr(self, i):
        return self.dbuf[self.alloc[i]].data_ptr() + self.es * self.base[i]

    def download(self):
        return [t.cpu().numpy().view(self.u) if t is not None else np.zeros(0, dtype=self.u) for t in self.dbuf]

    def upload(self):
        import torch
        for t, b in zip(self.dbuf, self.buf):
            if t is not None:
                t.copy_(torch.from_numpy(b.view({2: np.int16, 4: np.int32, 8: np.int64}[self.es])))


Lay = collections.namedtuple("Lay", "sharedB dupA second odd8", defaults=(False, False, False, False))
LAYOUTS = {
    "shared": Lay(sharedB=True),                         # one B, the same pointer repeated: the reference's call
    "perB": Lay(),                                       # a B per entry
    "dupA": Lay(dupA=True),                              # the last entry's A is entry 0's
    "second": Lay(second=True),                          # entries of every family in a second allocation
    "shared2": Lay(sharedB=True, dupA=True, second=True),
    "odd8": Lay(second=True, odd8=True),                 # f64 only: every base at 8 mod 16
    "odd8s": Lay(sharedB=True, odd8=True),
}


def draw(rng, kind, dtype, shape, k):
    n = int(np.prod(shape))
    if kind == "ties":
        v = rng.integers(-3, 4, n) if k <= 256 else rng.integers(-1, 2, n)
        return v.astype(dtype).reshape(shape)
    return rng.uniform(-1, 1, n).astype(dtype).reshape(shape)


class Problem:
    """One call: pools, index maps of the logical operands, references and -- after to_device() -- device copies and pointer tables.
    In the row-major view the logical operands are Bv [n][k] (op(B) transposed), Av [k][m] (op(A) transposed) and C [n][m]."""

    def __init__(self, entry, m, n, k, batch, ta=OP_N, tb=OP_N, lay=Lay(), ab=ABS[0], kind="uniform", rng=None, amap=None, bmap=None, nan_at=None):
        self.entry, self.sfx = entry, sfx_of(entry)
        self.m, self.n, self.k, self.batch, self.ta, self.tb, self.lay, self.kind = m, n, k, batch, ta, tb, lay, kind
        self.alpha, self.beta = ab
        d = self.d = DT[self.sfx]
        if amap is None:
            amap = list(range(batch))
            if lay.dupA and batch > 1:
                amap[-1] = 0
        if bmap is None:
            bmap = [0] * batch if lay.sharedB else list(range(batch))
        self.amap, self.bmap = list(amap), list(bmap)
        nA, nB = max(amap) + 1, max(bmap) + 1
        am, ak, an = np.arange(m), np.arange(k), np.arange(n)
        # stored element of Av[l][i] / Bv[j][l]: lda = m, ldb = k whatever the flags
        self.iA = (am[None, :] * m + ak[:, None]) if ta else (ak[:, None] * m + am[None, :])
        self.iB = (ak[None, :] * k + an[:, None]) if tb else (an[:, None] * k + ak[None, :])
        self.iC = an[:, None] * m + am[None, :]
        self.pA = Pool(self.sfx, int(self.iA.max()) + 1, nA, d["qnan"], lay.second, lay.odd8)
        self.pB = Pool(self.sfx, int(self.iB.max()) + 1, nB, d["qnan"], lay.second, lay.odd8)
        self.pC = Pool(self.sfx, n * m, batch, d["sent"], lay.second, lay.odd8)
        self.Av = draw(rng, kind, d["np"], (nA, k, m), k)
        self.Bv = draw(rng, kind, d["np"], (nB, n, k), k)
        self.C0v = draw(rng, kind, d["np"], (batch, n, m), k)
        if nan_at is not None:
            self.Av[nan_at] = np.nan
        self.expect_nan = nan_at is not None
        for i in range(nA):
            self.pA.scatter(i, self.iA, bits(self.Av[i]))
        for i in range(nB):
            self.pB.scatter(i, self.iB, bits(self.Bv[i]))
        self.reads_c = self.beta != 0.0
        for e in range(batch):
            self.pC.scatter(e, self.iC, bits(self.C0v[e]) if self.reads_c else np.full(n * m, d["sent"], dtype=d["u"]))
        self._ref = None

    def nbytes(self):
        return self.pA.nbytes() + self.pB.nbytes() + self.pC.nbytes()

    # ---- the reference: numpy in the wide type, distinct (A, B) pairs multiplied once ----------------
    def reference(self):
        """(ref, scale), [batch][n][m] in the wide type: alpha * Bv . Av + beta * C0 and |alpha| |Bv| . |Av| + |beta| |C0|."""
        key = (tuple(self.amap), tuple(self.bmap))
        if self._ref is None or self._ref[0] != key:
            W = self.d["wide"]
            A, B = self.Av.astype(W), self.Bv.astype(W)
            prods = {}
            for pair in set(zip(self.amap, self.bmap)):
                prods[pair] = (B[pair[1]] @ A[pair[0]], np.abs(B[pair[1]]) @ np.abs(A[pair[0]]))
            ref = np.stack([W(self.alpha) * prods[pr][0] for pr in zip(self.amap, self.bmap)])
            scale = np.stack([W(abs(self.alpha)) * prods[pr][1] for pr in zip(self.amap, self.bmap)])
            if self.reads_c:
                c0 = self.C0v.astype(W)
                ref, scale = ref + W(self.beta) * c0, scale + W(abs(self.beta)) * np.abs(c0)
            self._ref = (key, ref + W(0), scale)
        return self._ref[1], self._ref[2]

    def assert_ties_premise(self):
        """Small integers, alpha and beta powers of two: the wide result is a value of the output type, and every partial sum of
        the kernels (fp32 for f16 / f32, fp64 for f64) is an integer below 2^24."""
        assert self.kind == "ties" and (self.alpha, self.beta) in ABS
        ref, scale = self.reference()
        assert np.array_equal(ref.astype(self.d["np"]).astype(self.d["wide"]), ref) and float(scale.max()) < 2.0 ** 24

    # ---- device ---------------------------------------------------------------------------------
    def to_device(self):
        import torch
        for p in (self.pA, self.pB, self.pC):
            p.to_device()
        self.tA, self.tB, self.tC = (torch.zeros(self.batch, dtype=torch.int64, device="cuda") for _ in range(3))
        self.write_tables()
        return self

    def tables(self):
        return ([self.pA.ptr(i) for i in self.amap], [self.pB.ptr(i) for i in self.bmap], [self.pC.ptr(e) for e in range(self.batch)])

    def write_tables(self, amap=None, bmap=None):
        """The pointer tables, rewritten in device memory (the tensors -- and so the addresses a captured call holds -- stay)."""
        import torch
        if amap is not None:
            self.amap, self.bmap = list(amap), list(bmap)
        for t, ptrs in zip((self.tA, self.tB, self.tC), self.tables()):
            t.copy_(torch.tensor(ptrs, dtype=torch.int64))

    def reset_c(self):
        self.pC.upload()

    def result(self, what):
        """The logical C entries as bits [batch][n][m], after asserting that every guard and gap word of C kept its bits and that A and B
        are unchanged."""
        import torch
        torch.cuda.synchronize()
        got = self.pC.download()
        for a, (g, h, lg) in enumerate(zip(got, self.pC.buf, self.pC.logical)):
            changed = np.flatnonzero(~lg & (g != h))
            assert changed.size == 0, f"{what}: {changed.size} guard / gap words of C (allocation {a}) were written, first at {changed[:8]}"
        for name, pool in (("A", self.pA), ("B", self.pB)):
            for g, h in zip(pool.download(), pool.buf):
                assert np.array_equal(g, h), f"{what}: {name} was modified"
        return np.stack([self.pC.gather(e, self.iC, got) for e in range(self.batch)])

    def check(self, what, got, upto=None):
        """upto: the call ran the first `upto` entries of the tables only."""
        ref, scale = self.reference()
        if upto is not None:
            got, ref, scale = got[:upto], ref[:upto], scale[:upto]
        g = got.view(self.d["np"])
        gn, rn = np.isnan(g), np.isnan(ref.astype(np.float64))
        bad = np.argwhere(gn & ~rn)
        assert bad.size == 0, f"{what}: {len(bad)} NaN results (padding or the sentinel read into a result?), first at (entry, col, row) {bad[:4].tolist()}"
        bad = np.argwhere(rn & ~gn)
        assert bad.size == 0, f"{what}: {len(bad)} results miss the NaN of their operand, first at (entry, col, row) {bad[:4].tolist()}"
        assert self.expect_nan == bool(rn.any())
        ok = ~rn
        if self.kind == "ties":
            want = bits(ref.astype(self.d["np"]))
            for e in range(len(g)):
                wrong = np.argwhere((got[e] != want[e]) & ok[e])
                assert wrong.size == 0, f"{what}: entry {e}: {len(wrong)} results are not the exact product, first at (col, row) {wrong[:4].tolist()}"
            return
        tol = self.d["tol"]
        r64, s64 = ref.astype(np.float64), scale.astype(np.float64)
        for e in range(len(g)):
            err = np.abs(g[e].astype(self.d["wide"]) - ref[e]).astype(np.float64)
            out = np.argwhere((err > tol * np.maximum(s64[e], 1e-30)) & ok[e])
            assert out.size == 0, f"{what}: entry {e}: {len(out)} results outside {tol}, first at (col, row) {out[:4].tolist()}"
        check_close(g[ok], r64[ok], s64[ok], tol, what, self.k, self.sfx)


# ---------------------------------------------------------------------------------------------
# the entry points through the C ABI (pointers as integers: the refusals are called without a device too)
# ---------------------------------------------------------------------------------------------
def call_entry(L, entry, tA, tB, tC, m, n, k, batch, ta, tb, alpha, beta, ws=None, ws_bytes=0, stream=None):
    if entry == "f16":
        return L.sm_gemm_batched_f16(tA, tB, tC, m, n, k, batch, ta, tb, alpha, beta, stream)
    if entry == "f16_ws":
        return L.sm_gemm_batched_f16_ws(tA, tB, tC, m, n, k, batch, ta, tb, alpha, beta, ws, ws_bytes, stream)
    return getattr(L, "sm_gemm_batched_" + entry)(tA, tB, tC, m, n, k, batch, ta, tb, alpha, beta, stream)


def run(gpu, p, entry=None, ws=None, stream=None, batch=None):
    L = gpu.lib()
    rc = call_entry(L, entry or p.entry, p.tA.data_ptr(), p.tB.data_ptr(), p.tC.data_ptr(), p.m, p.n, p.k, p.batch if batch is None else batch, p.ta, p.tb,
                    p.alpha, p.beta, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), stream)
    assert rc == 0, f"{entry or p.entry}: status {rc}: {L.sm_last_error().decode()}"


def sk_workspace(need_bytes):
    """A stream-K workspace of exactly `need_bytes`: a zero flag page (sm_spmma_fused_workspace_state: the first 4 KiB must be clean
    before a call), garbage behind it -- a slot the kernel wrote shows (test_gpu_parity.test_fused_streamk_vs_oracle)."""
    import torch
    ws = torch.zeros(max(need_bytes, 4096 + 16), dtype=torch.uint8, device="cuda")
    ws[4096:].fill_(0xff)
    assert ws.data_ptr() % 16 == 0
    return ws


# ---------------------------------------------------------------------------------------------
# the dispatch rules, mirrored in the call's (m, n, k, batch, ta, tb) -- test_gemm_batched_cases.py holds every case against them
# ---------------------------------------------------------------------------------------------
def span_lds_fits(m, k):
    """spmma_f16_fused.hip, span_lds_fits(n = m, k): the span of 128 rows and the whole B, k rounded up to 64, inside 160 KiB."""
    return 128 * k * 2 + 1152 + (k + 63) // 64 * 64 * (64 if m <= 64 else 128) * 2 <= 160 * 1024


def _sk_cuts(tiles, wg, nkt, lead):
    total = float(tiles * nkt)
    x = [total / wg] * wg
    cut = [0] * 9
    for _ in range(6):
        acc = 0.0
        for r in range(wg):
            acc += x[r]
            cut[r + 1] = int(total) if r + 1 == wg else int(acc + 0.5)
        shrt = []
        for r in range(wg):
            last_tile = ((cut[r + 1] - 1) & 0xffffffff) // nkt
            seg0 = max(cut[r], last_tile * nkt)
            shrt.append(cut[r + 1] > cut[r] and seg0 != last_tile * nkt)
        T = (total + float(lead) * sum(shrt)) / wg
        if T - lead < 2.0:
            break
        x = [T - lead if s else T for s in shrt]
    longest = 0
    for r in range(wg):
        cut[r + 1] = max(cut[r + 1], cut[r])
        longest = max(longest, cut[r + 1] - cut[r])
    return longest


def sk_plan(panels, nkt, tn, cus):
    """spmma_f16_fused.hip, sk_plan: (slots, wg, units) of the chosen decomposition, slots == 0: none."""
    best = (0, 0, 0)
    max_slots = cus // tn
    if max_slots == 0 or panels == 0 or nkt == 0 or nkt > 0xffff:
        return best
    for wg in range(1, 9):
        for tg in range(1, 17):
            if wg > 1 and tg * nkt < 2 * wg:
                continue
            gf, tgl = divmod(panels, tg)
            wgl = (tgl * wg + tg - 1) // tg if tgl else 0
            if gf * wg + wgl == 0 or gf * wg + wgl > max_slots:
                continue
            units = _sk_cuts(tg, wg, nkt, 3) if gf else 0
            if tgl:
                units = max(units, _sk_cuts(tgl, wgl, nkt, 3))
            if best[0] == 0 or units < best[2]:
                best = (gf * wg + wgl, wg, units)
    return best


def sk_takes(rows, problems, cols, k, cus):
    """spmma_f16_fused.hip, sk_takes (no A-stationary shape): (taken, workspace bytes the launch needs)."""
    if cols <= 128 or k < 128 or k % 64 != 0:
        return False, 0
    nkt, tn = k // 64, (cols + 255) // 256
    panels = (rows + 255) // 256 * problems
    t_big, t_wide = panels * tn, (rows + 127) // 128 * tn * problems
    slots, wg, units = sk_plan(panels, nkt, tn, cus)
    if not slots:
        return False, 0
    c_sk = units + (8.0 if wg > 1 else 0.0)
    c_now = min(float((t_big + cus - 1) // cus * nkt), 0.6 * float((t_wide + cus - 1) // cus * nkt))
    return wg > 1 and c_sk < 0.85 * c_now, 4096 + slots * tn * 256 * 256 * 4


def facts(entry, m, n, k, batch, ta, tb, cus=256):
    f = dict(entry=entry, m=m, n=n, k=k, batch=batch, ta=ta, tb=tb, tr=bool(ta or tb))
    if entry == "f64":
        f["mc"] = not f["tr"] and k % 16 == 0 and k >= 16 and m % 2 == 0 and m >= 2 and (n + 63) // 64 <= 65535
        f["big"] = n > 64 and m > 64 and 4 * ((n + 127) // 128) * ((m + 127) // 128) * batch >= 3 * cus
    elif entry == "f32":
        f["dma"] = not tb and k % 32 == 0 and k >= 32 and m % 4 == 0 and m >= 4
        f["tile"] = ("64,64" if m <= 64 else "64,128") if n <= 64 else ("128,64" if m <= 128 else "128,128")
        f["big"] = ((n + 63) // 64) * ((m + 63) // 64) * batch >= 32 * cus
    else:
        f["vec"] = 8 if k % 8 == 0 and m % 8 == 0 else 4 if k % 4 == 0 and m % 4 == 0 else 1
        ragged = k % 64 != 0
        twin_ok = not f["tr"] and m % 8 == 0 and m >= 8
        f["span"] = twin_ok and ragged and m <= 128 and (n * k) % 8 == 0 and span_lds_fits(m, k)
        f["bigshape"] = twin_ok and not ragged and 128 < m <= 256 and k >= 2048
        f["big"] = f["bigshape"] and (n + 255) // 256 * 256 * 100 <= n * 115
        f["sk"] = entry == "f16_ws" and f["bigshape"] and sk_takes(n, batch, m, k, cus)[0]
        twin = f["span"] or f["big"] or f["sk"]
        f["fast"] = not f["tr"] and not twin and k % 64 == 0 and m % 4 == 0 and m >= 8
        f["cfg"] = not f["tr"] and not twin and not f["fast"]
        f["tile"] = "128,64" if m <= 64 else "64,128" if n <= 64 else "128,128"
    return f


CLASS_NEEDS = {
    "f64": {
        "f64 dma<64,64>": lambda f: f["mc"] and not f["big"],
        "f64 dma<128,128>": lambda f: f["mc"] and f["big"],
        "f64 fma": lambda f: not f["mc"],
    },
    "f32": dict(
        [(f"f32 dma<{t}>", lambda f, t=t: f["dma"] and not f["ta"] and f["tile"] == t) for t in ("64,64", "64,128", "128,64", "128,128")] +
        [(f"f32 T dma<{t}>", lambda f, t=t: f["dma"] and f["ta"] and f["tile"] == t) for t in ("64,64", "64,128", "128,64", "128,128")] +
        [("f32 generic<64,64>", lambda f: not f["tr"] and not f["dma"] and not f["big"]),
         ("f32 generic<128,64>", lambda f: not f["tr"] and not f["dma"] and f["big"]),
         ("f32 T generic<64,64>", lambda f: f["ta"] and not f["tb"] and not f["dma"] and not f["big"]),
         ("f32 atr<0>", lambda f: f["tb"] and not f["ta"]),
         ("f32 atr<2>", lambda f: f["tb"] and f["ta"])]),
    "f16": dict(
        [("twin span<64>", lambda f: f["span"] and f["m"] <= 64),
         ("twin span<128>", lambda f: f["span"] and f["m"] > 64),
         ("twin big<256>", lambda f: f["big"])] +
        [(f"dma<{t}>", lambda f, t=t: f["fast"] and f["tile"] == t) for t in ("128,64", "64,128", "128,128")] +
        [(f"cfg<{t}> vec{v}", lambda f, t=t, v=v: f["cfg"] and f["tile"] == t and f["vec"] == v) for t in ("128,64", "64,128", "128,128") for v in (8, 4, 1)] +
        [("cfg<128,128,T> vec8", lambda f: f["tr"] and f["vec"] == 8),
         ("cfg<128,128,T> vec4->1", lambda f: f["tr"] and f["vec"] == 4),
         ("cfg<128,128,T> vec1", lambda f: f["tr"] and f["vec"] == 1)]),
    "f16_ws": {
        "twin streamk": lambda f: f["sk"],
        "ws twin big<256>": lambda f: f["big"] and not f["sk"],
    },
}


def classes_of(entry, m, n, k, batch, ta, tb, cus=256):
    f = facts(entry, m, n, k, batch, ta, tb, cus)
    return [cls for cls, need in CLASS_NEEDS[entry].items() if need(f)]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "entry cls m n k batch ta tb lname ab")


def _cases(entry, rows, layouts):
    """rows: (class, m, n, k[, batch[, ta, tb]]); the layouts walk the rows, the two (alpha, beta) the rows of each class."""
    out, seen = [], collections.Counter()
    for i, row in enumerate(rows):
        cls, m, n, k = row[:4]
        batch = row[4] if len(row) > 4 else 2 + (seen[cls] // 2 + i) % 2
        ta, tb = row[5:7] if len(row) > 5 else (OP_N, OP_N)
        out.append(Case(entry, cls, m, n, k, batch, ta, tb, layouts[i % len(layouts)], seen[cls] % 2))
        seen[cls] += 1
    return out


F64_CASES = _cases("f64", [("f64 dma<64,64>", m, n, (16, 32, 48)[(i + j) % 3]) for i, m in enumerate((2, 66, 130)) for j, n in enumerate((40, 64, 65, 200))] +
                   [("f64 dma<64,64>", 130, 200, 16), ("f64 dma<64,64>", 130, 200, 32), ("f64 dma<64,64>", 66, 65, 48), ("f64 dma<64,64>", 2, 200, 48)] +
                   [("f64 fma", 67, 33, 5), ("f64 fma", 67, 33, 24), ("f64 fma", 67, 70, 16), ("f64 fma", 66, 130, 24),
                    ("f64 fma", 67, 33, 40, 2, OP_T, OP_N), ("f64 fma", 67, 33, 40, 3, OP_N, OP_T), ("f64 fma", 67, 33, 40, 2, OP_T, OP_T),
                    ("f64 fma", 66, 30, 48, 2, OP_T, OP_N)],
                  ("shared", "odd8", "perB", "dupA", "odd8s", "second", "shared2"))

_F32_DMA = [("64,64", 40, 40), ("64,128", 72, 40), ("64,128", 200, 40), ("128,64", 40, 200), ("128,64", 104, 200), ("128,128", 136, 200)]
F32_CASES = _cases("f32", [(f"f32 dma<{t}>", m, n, k) for t, m, n in _F32_DMA for k in (32, 64, 160)] +
                   [("f32 generic<64,64>", 37, 200, 72), ("f32 generic<64,64>", 37, 200, 64), ("f32 generic<64,64>", 40, 70, 5), ("f32 generic<64,64>", 131, 35, 77)] +
                   # ta = T needs m >= k (so <64,64> has two k stages at m = 64 only)
                   [("f32 T dma<64,64>", 40, 40, 32, 2, OP_T, OP_N), ("f32 T dma<64,64>", 64, 40, 64, 3, OP_T, OP_N),
                    ("f32 T dma<64,128>", 72, 40, 64, 2, OP_T, OP_N), ("f32 T dma<64,128>", 200, 40, 160, 3, OP_T, OP_N),
                    ("f32 T dma<128,64>", 40, 200, 32, 2, OP_T, OP_N), ("f32 T dma<128,64>", 104, 200, 64, 3, OP_T, OP_N),
                    ("f32 T dma<128,128>", 136, 200, 64, 2, OP_T, OP_N), ("f32 T dma<128,128>", 200, 200, 160, 3, OP_T, OP_N),
                    ("f32 T generic<64,64>", 131, 70, 72, 2, OP_T, OP_N), ("f32 T generic<64,64>", 37, 70, 32, 3, OP_T, OP_N),
                    ("f32 T generic<64,64>", 200, 35, 5, 2, OP_T, OP_N)] +
                   # tb = T needs k >= n
                   [("f32 atr<0>", 131, 70, 77, 2, OP_N, OP_T), ("f32 atr<0>", 40, 35, 72, 3, OP_N, OP_T),
                    ("f32 atr<2>", 131, 70, 77, 2, OP_T, OP_T), ("f32 atr<2>", 72, 35, 64, 3, OP_T, OP_T)],
                  ("shared", "perB", "dupA", "second", "shared2"))

F16_CASES = _cases("f16", [(f"twin span<{64 if m <= 64 else 128}>", m, 200, k, b) for m in (40, 104) for k in (72, 147) for b in (3, 11)] +
                   [("twin big<256>", 136, 250, 2048, 2), ("twin big<256>", 256, 250, 2048, 2)] +
                   [("dma<128,64>", 40, 200, 64), ("dma<128,64>", 36, 200, 192), ("dma<128,64>", 36, 40, 64), ("dma<128,64>", 40, 200, 192),
                    ("dma<64,128>", 104, 40, 64), ("dma<64,128>", 132, 40, 192), ("dma<64,128>", 132, 40, 64), ("dma<64,128>", 104, 40, 192),
                    ("dma<128,128>", 104, 200, 64), ("dma<128,128>", 132, 200, 192), ("dma<128,128>", 136, 200, 128), ("dma<128,128>", 132, 200, 64)] +
                   [("cfg<128,64> vec8", 40, 200, 440), ("cfg<128,64> vec8", 64, 70, 440),
                    ("cfg<64,128> vec8", 136, 40, 72), ("cfg<64,128> vec8", 200, 64, 200),
                    ("cfg<128,128> vec8", 136, 200, 72), ("cfg<128,128> vec8", 264, 70, 200),
                    ("cfg<128,64> vec4", 36, 200, 72), ("cfg<128,64> vec4", 40, 35, 76),
                    ("cfg<64,128> vec4", 132, 40, 72), ("cfg<64,128> vec4", 136, 35, 76),
                    ("cfg<128,128> vec4", 132, 200, 72), ("cfg<128,128> vec4", 136, 201, 76),
                    ("cfg<128,64> vec1", 37, 200, 72), ("cfg<128,64> vec1", 40, 201, 147),
                    ("cfg<64,128> vec1", 130, 40, 200), ("cfg<64,128> vec1", 131, 40, 147),
                    ("cfg<128,128> vec1", 130, 200, 200), ("cfg<128,128> vec1", 136, 201, 147)] +
                   # ta = T needs m >= k, tb = T needs k >= n
                   [("cfg<128,128,T> vec8", 136, 40, 72, 2, ta, tb) for ta, tb in ((OP_T, OP_N), (OP_N, OP_T), (OP_T, OP_T))] +
                   [("cfg<128,128,T> vec8", 264, 136, 200, 3, OP_T, OP_T)] +
                   [("cfg<128,128,T> vec4->1", 136, 40, 76, 2, ta, tb) for ta, tb in ((OP_T, OP_N), (OP_N, OP_T), (OP_T, OP_T))] +
                   [("cfg<128,128,T> vec4->1", 132, 40, 72, 3, ta, tb) for ta, tb in ((OP_T, OP_N), (OP_N, OP_T), (OP_T, OP_T))] +
                   [("cfg<128,128,T> vec1", 131, 35, 77, 2, ta, tb) for ta, tb in ((OP_T, OP_N), (OP_N, OP_T), (OP_T, OP_T))],
                  ("shared", "perB", "dupA", "second", "shared2"))

# the workspace entry point: the same big-form shapes.  At 256 CUs the plan takes every batch up to 42 and declines from SK_DECLINED on
# (whole tiles then fill the rounds); elsewhere the device's plan decides which of the two classes a case runs
SK_BATCH, SK_DECLINED = 3, 43
WS_CASES = _cases("f16_ws", [("ws twin big<256>", 136, 250, 2048, SK_DECLINED), ("ws twin big<256>", 136, 250, 2048, SK_DECLINED + 1),
                             ("twin streamk", 136, 250, 2048, 2), ("twin streamk", 256, 250, 2048, SK_BATCH)], ("shared", "shared", "second", "dupA"))
ALL_CASES = F64_CASES + F32_CASES + F16_CASES + WS_CASES


def _cid(c):
    return f"{c.cls.replace(' ', '_')}-{c.m}x{c.n}x{c.k}x{c.batch}-{'NT'[c.ta]}{'NT'[c.tb]}-{c.lname}-ab{c.ab}"


def problem_of(c, kind, **kw):
    return Problem(c.entry, c.m, c.n, c.k, c.batch, c.ta, c.tb, LAYOUTS[c.lname], ABS[c.ab], kind,
                   np.random.default_rng(_seed(kind, c.entry, c.m, c.n, c.k, c.batch, c.ta, c.tb, c.lname, c.ab)), **kw)


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(gpu, c, ws=None):
    for kind in KINDS:
        p = problem_of(c, kind)
        if kind == "ties":
            p.assert_ties_premise()
        run(gpu, p.to_device(), ws=ws)
        what = f"sm_gemm_batched_{c.entry} {kind} {_cid(c)}"
        p.check(what, p.result(what))


@pytest.mark.parametrize("case", F64_CASES + F32_CASES + F16_CASES, ids=_cid)
def test_pointer_arrays_on_guarded_operands(gpu, case):
    assert classes_of(*case[:1], *case[2:8], cus=device_cus()) == [case.cls], "the case does not reach its class on this device"
    run_case(gpu, case)


@pytest.mark.parametrize("case", WS_CASES, ids=_cid)
def test_ws_entry_stream_k_or_big_as_the_plan_says(gpu, case):
    """sm_gemm_batched_f16_ws: the stream-K twin where sm_spmma_fused_streamk_plan (rows n, columns m, k, batch problems) says so on this
    device -- slots of the workspace are then written and the flag page comes back clean -- and the big form, workspace untouched, where not."""
    cus = device_cus()
    takes_lib, plan = gpu.spmma_fused_streamk_plan(case.n, case.m, case.k, case.batch)
    takes, need = sk_takes(case.n, case.batch, case.m, case.k, cus)
    assert takes == takes_lib and (not takes or need == 4096 + plan["slots"] * 256 * 256 * 4), "the mirror of sk_takes disagrees with the library"
    if cus == 256:
        assert takes == (case.cls == "twin streamk")
    for kind in KINDS:
        p = problem_of(case, kind)
        if kind == "ties":
            p.assert_ties_premise()
        ws = sk_workspace(need)
        run(gpu, p.to_device(), ws=ws)
        what = f"sm_gemm_batched_f16_ws {kind} {_cid(case)}"
        p.check(what, p.result(what))
        assert bool((ws[4096:] != 0xff).any().item()) == takes, "stream-K ran" if not takes else "the shape was meant to take the stream-K kernel"
        assert gpu.spmma_fused_workspace_state(ws) == 0, "flags not handed back as zero"


@pytest.mark.parametrize("how", ["none", "small"])
def test_ws_entry_without_a_usable_workspace_is_the_plain_call(gpu, how):
    """A null workspace, or one smaller than the plan needs, runs what sm_gemm_batched_f16 runs: the big form, the same bits."""
    c = WS_CASES[-1]
    p = problem_of(c, "uniform").to_device()
    run(gpu, p, entry="f16")
    plain = p.result("plain")
    p.check(f"sm_gemm_batched_f16 uniform {_cid(c)} (plain, for the workspace forms)", plain)
    p.reset_c()
    takes, need = sk_takes(c.n, c.batch, c.m, c.k, device_cus())
    ws = None if how == "none" else sk_workspace((need if takes else 4096 + 256 * 256 * 4) - 16)
    run(gpu, p, ws=ws)
    got = p.result(f"workspace {how}")
    assert np.array_equal(got, plain), f"workspace {how}: differs from the call without a workspace"
    assert ws is None or not bool((ws[4096:] != 0xff).any().item()), "a workspace that is too small was written"


# ---- classes whose batch comes from the CU count
def f64_big_shape(cus):
    """(m, n, batch): 4 * (2 x 2 tiles of 128 x 128) * batch >= 3 * cus, and not one entry below."""
    return 200, 200, (3 * cus + 15) // 16


F64_BIG_LAYOUT = {16: "odd8", 48: "second"}   # k -> layout: the 128 x 128 tiling with every base at 8 mod 16 too

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [16, 48])
def test_f64_big_tiles(gpu, k, kind):
    """gemm_f64_dma_kernel<128,128,4,4>: taken from 3/4 of the CUs in big tiles on.  A few distinct A and B, every C distinct; the same
    operands one entry below the threshold run the 64 x 64 class.  Each run against the reference (no contract makes the two agree bit for bit)."""
    cus = device_cus()
    m, n, batch = f64_big_shape(cus)
    assert classes_of("f64", m, n, k, batch, 0, 0, cus) == ["f64 dma<128,128>"] and classes_of("f64", m, n, k, batch - 1, 0, 0, cus) == ["f64 dma<64,64>"]
    p = Problem("f64", m, n, k, batch, lay=LAYOUTS[F64_BIG_LAYOUT[k]], ab=ABS[k == 48], kind=kind, rng=np.random.default_rng(_seed("f64big", k, kind)),
                amap=[e % 3 for e in range(batch)], bmap=[e % 2 for e in range(batch)])
    assert p.nbytes() < CAP_BYTES * max(1.0, cus / 256.0)
    if kind == "ties":
        p.assert_ties_premise()
    p.to_device()
    for b, cls in ((batch, "dma<128,128>"), (batch - 1, "dma<64,64>")):
        run(gpu, p, batch=b)
        got = p.result(f"f64 {cls}")
        if b < batch:   # the entry the shorter call leaves out keeps what C held
            assert np.array_equal(got[batch - 1], p.pC.gather(batch - 1, p.iC)), "an entry beyond `batch` was written"
        p.check(f"sm_gemm_batched_f64 {kind} {cls} (m, n, k, batch) = {(m, n, k, b)}", got, upto=b)
        p.reset_c()


def f32_generic_big_shape(cus):
    """(m, n, k, batch): 3 x 1 tiles of 64 x 64 per entry, 32 per CU; a thin k of two steps that is no multiple of 32, ragged in both directions."""
    return 5, 130, 40, (32 * cus + 2) // 3


@pytest.mark.parametrize("kind", KINDS)
def test_f32_generic_128x64(gpu, kind):
    cus = device_cus()
    m, n, k, batch = f32_generic_big_shape(cus)
    assert classes_of("f32", m, n, k, batch, 0, 0, cus) == ["f32 generic<128,64>"]
    p = Problem("f32", m, n, k, batch, lay=LAYOUTS["second"], ab=ABS[kind == "ties"], kind=kind, rng=np.random.default_rng(_seed("f32big", kind)),
                amap=[e % 3 for e in range(batch)], bmap=[e % 2 for e in range(batch)])
    assert p.nbytes() < CAP_BYTES * max(1.0, cus / 256.0)
    if kind == "ties":
        p.assert_ties_premise()
    run(gpu, p.to_device())
    what = f"sm_gemm_batched_f32 {kind} generic<128,64> (m, n, k, batch) = {(m, n, k, batch)}"
    p.check(what, p.result(what))


# ---- once per entry point: (m, n, k) of a small case of a matrix-core class
ONCE = {"f16": (104, 200, 147), "f16_ws": (136, 250, 2048), "f32": (136, 200, 64), "f64": (130, 200, 32)}


def _ws_for(entry, m, n, k, batch):
    takes, need = sk_takes(n, batch, m, k, device_cus())
    return sk_workspace(need if takes else 4096 + 16) if entry == "f16_ws" else None


@pytest.mark.parametrize("entry", ENTRIES)
def test_nan_in_one_a_reaches_the_entries_that_name_it(gpu, entry):
    """A NaN at A[l0][i0] of matrix 0, which entries 0 and 2 name (dupA): column i0 of C (row-major view) of exactly those entries."""
    m, n, k = ONCE[entry]
    batch = SK_BATCH if entry == "f16_ws" else 3
    for ab in ABS:
        p = Problem(entry, m, n, k, batch, lay=LAYOUTS["dupA"], ab=ab, kind="uniform", rng=np.random.default_rng(_seed("nan", entry, ab[0])), nan_at=(0, k - 3, m - 2))
        ref, _ = p.reference()
        want = np.zeros((batch, n, m), dtype=bool)
        want[[0, batch - 1], :, m - 2] = True
        assert np.array_equal(np.isnan(ref.astype(np.float64)), want)
        run(gpu, p.to_device(), ws=_ws_for(entry, m, n, k, batch))
        what = f"sm_gemm_batched_{entry} NaN in A, (alpha, beta) = {ab}"
        p.check(what, p.result(what))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_batch_of_one(gpu, entry, kind):
    m, n, k = ONCE[entry]
    p = Problem(entry, m, n, k, 1, lay=LAYOUTS["perB"], ab=ABS[kind == "uniform"], kind=kind, rng=np.random.default_rng(_seed("one", entry, kind)))
    if kind == "ties":
        p.assert_ties_premise()
    run(gpu, p.to_device(), ws=_ws_for(entry, m, n, k, 1))
    what = f"sm_gemm_batched_{entry} {kind} batch 1 {(m, n, k)}"
    p.check(what, p.result(what))


@pytest.mark.parametrize("entry", ENTRIES)
def test_graph_replays_follow_the_pointer_tables(gpu, entry):
    """Captured once (one stream: a chain of kernel nodes, no parallel branches); the pointer tables then change in device memory only,
    and every replay equals the eager run of its table."""
    import ctypes
    import torch
    m, n, k = ONCE[entry]
    batch = SK_BATCH if entry == "f16_ws" else 3
    p = Problem(entry, m, n, k, batch, lay=LAYOUTS["second"], ab=ABS[1], kind="uniform", rng=np.random.default_rng(_seed("graph", entry))).to_device()
    ws = _ws_for(entry, m, n, k, batch)
    ident = list(range(batch))
    maps = [(ident, ident), (ident[1:] + ident[:1], ident[2:] + ident[:2]), ([0] * batch, ident[::-1])]
    eager = []
    for am, bm in maps:
        p.write_tables(am, bm)
        p.reset_c()
        run(gpu, p, ws=ws)
        got = p.result(f"eager {am}")
        p.check(f"sm_gemm_batched_{entry} uniform eager, tables {am} {bm}", got)
        eager.append(got)
    assert not np.array_equal(eager[0], eager[1]) and not np.array_equal(eager[1], eager[2])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(gpu, p, ws=ws, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    for (am, bm), want in list(zip(maps, eager)) + [(maps[0], eager[0])]:
        p.write_tables(am, bm)
        p.reset_c()
        graph.replay()
        assert np.array_equal(p.result(f"replay {am}"), want), f"replay under tables {am} {bm} differs from the eager run"


# ---------------------------------------------------------------------------------------------
# refusals: decided before any device work (also called without a device by test_gemm_batched_cases.py)
# ---------------------------------------------------------------------------------------------
BIG = 1 << 31
# name -> (entries, (m, n, k, batch, ta, tb), null tables?, status)
REFUSALS = {
    "null tables": (ENTRIES, (8, 8, 8, 1, OP_N, OP_N), True, INVALID),
    "operation 2": (ENTRIES, (8, 8, 8, 1, 2, OP_N), False, INVALID),
    "operation -1": (ENTRIES, (8, 8, 8, 1, OP_N, -1), False, INVALID),
    "ta = T, m < k": (ENTRIES, (8, 8, 16, 1, OP_T, OP_N), False, INVALID),
    "tb = T, k < n": (ENTRIES, (32, 16, 8, 1, OP_N, OP_T), False, INVALID),
    "f64 batch 65536": (("f64",), (8, 8, 8, 65536, OP_N, OP_N), False, NOT_SUPPORTED),
    "m = 2^31": (ENTRIES, (BIG, 8, 8, 1, OP_N, OP_N), False, NOT_SUPPORTED),
    "n = 2^31": (ENTRIES, (8, BIG, 8, 1, OP_N, OP_N), False, NOT_SUPPORTED),
    "k = 2^31": (ENTRIES, (8, 8, BIG, 1, OP_N, OP_N), False, NOT_SUPPORTED),
    "empty m": (ENTRIES, (0, 8, 8, 1, OP_N, OP_N), False, 0),
    "empty n": (ENTRIES, (8, 0, 8, 1, OP_N, OP_N), False, 0),
    "empty batch": (ENTRIES, (8, 8, 8, 0, OP_N, OP_N), False, 0),
}


def refusal_status(L, entry, name, table):
    """The status of REFUSALS[name] for `entry`; table: a non-null address that is passed for every pointer array (and never read)."""
    _, dims, null, _ = REFUSALS[name]
    statuses = []
    for nulls in ([(0, 1, 1), (1, 0, 1), (1, 1, 0)] if null else [(1, 1, 1)]):
        tA, tB, tC = (table if x else None for x in nulls)
        statuses.append(call_entry(L, entry, tA, tB, tC, *dims, 1.0, 0.0, table, 1 << 30, None))
    assert len(set(statuses)) == 1
    return statuses[0]


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_and_empty_extents_leave_c_alone(gpu, name):
    p = Problem("f32", 8, 8, 16, 2, kind="uniform", rng=np.random.default_rng(_seed(name))).to_device()
    entries, _, _, status = REFUSALS[name]
    for entry in entries:
        assert refusal_status(gpu.lib(), entry, name, p.tC.data_ptr()) == status, f"{name}: {entry}"
    got = p.result(name)
    assert np.array_equal(got, np.full_like(got, DT["f32"]["sent"])), f"{name}: C was written"


# ---------------------------------------------------------------------------------------------
# margins of this file's `uniform` comparisons, appended to the session's report: the worst per entry point, then the worst cases
# ---------------------------------------------------------------------------------------------
_gemm_batched_margin_report = margin_report_fixture(
    "{n} comparisons of tests/test_gpu_gemm_batched.py against the numpy fp64 / longdouble product; err / bound (check_close), worst per entry point:",
    per_first_word=True)
