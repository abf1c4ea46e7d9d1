"""The exact fp32 Blocked-ELL and COO products of csrc/spmm.hip on GUARDED operands, per launch class (-m gpu).

Every input lies between guards that poison an over-read (quiet NaN around values / vals / B, ~0 around column_indices, index 0 around the COO
rows / cols so that an entry read past nnz lands in row 0 with the NaN of the vals guard), every C lies inside a larger allocation of 0x5A5A5A5A
words (64 in front of and behind each C; the batched Blocked-ELL table lists its Cs in a shuffled order with unequal gaps), every workspace has
exactly the bytes the library's *_workspace_size reports, pre-filled with 0x5A and followed by a guard.  Afterwards the guards, the inputs and
the bytes around the workspace must hold what they held.  With beta == 0 C starts as quiet NaN and must come out NaN-free.  The values of an EMPTY
Blocked-ELL block are NaN as well: nothing may read them.

The references are NOT the library: numpy fp64 from the definition (Blocked-ELL: the blocks densified, a block id >= cols / block_size skipped; COO:
np.add.at into a dense A, duplicates adding, coordinates out of range skipped), alpha and beta applied in fp64.  Two data kinds per case: `ties`
(integers in [-3, 3], (alpha, beta) in {(1, 0), (0.5, -2)}: every partial sum is a multiple of 0.5 below 2^24 -- asserted -- so the fp32 result is
exact in ANY summation order, atomics included, and ALL of C must equal the reference; +0 and -0 compare equal: beta * (+0) is -0 where C is scaled
first and +0 where the scaling is fused into the store) and `uniform` (U(-1, 1): check_close of parity_testlib at FP32_TOL and the rounding +
accumulation bound, k = the longest row's term count + 2).

Launch classes and the cases that pin them (tests/test_spmm32_cases.py restates every rule and holds every case against it):

    Blocked-ELL expansion (spmm.hip: launch_bell_expand)      cases
    expand, 16-byte stores   cols * 4 <= 48 KiB, cols % 4 == 0  cols = 12288 (the last that takes it) and every dispatch case
    expand, element stores   cols % 4 != 0, or workspace + 4 B  cols = 50; ws+4 (sm_spmm_bell_f32_ws only: the tables of the batched form are pointers)
    memset + scatter         cols * 4 > 48 KiB                  cols = 12320 (then the DMA GEMM), 12292 (then the generic GEMM), ell_cols = 0 on it
    dispatch32<2> (gemm_f32.hip), (M, N, K) = (n, rows, cols)
    dma<64,64> dma<64,128> dma<128,64> dma<128,128>             the issue's four shapes, each with cols 64, 32 (one stage) and 160; both sides of n 64 / 68,
                                                                rows 64 / 68 and rows 128 / 132
    generic<64,64>           cols % 32 != 0; B + one float      (40, 40, 72); (40, 40, 64) with b_off = 1; ws+4
    generic<128,64>          >= 32 small tiles per CU           the batched form sized from the CU count: test_bell_generic_128x64_tiles
    stores                   vector: aligned C, rows % 4 == 0; per element: C + one float, odd rows
    structure                block_size 1, 2, 3, 4, 8; rows % bs != 0; cols % bs != 0; empty blocks (~0 and cols / bs, middle and end); descending and
                             shuffled blocks; ell_cols == 0; n 1, 8, 9 (BELL_J = 8); rows 255, 256, 257 -- all through the three entry points, batch 3

    COO (spmm.hip)           entry       A_cols               flag word (first int of the workspace, read back and asserted)
    ws J32 / J16 / J8        _ws         <= 576 / 2304 / 4608  0 (spmm_csr_lds_kernel<J>)
    ws row                   _ws         >= 4609               0 (thread-per-row spmm_csr_kernel)
    packed J32 / J16         _packed     <= 639 / 2559         4 (spmm_csr_packed_kernel<J>)
    packed->ws               _packed     >= 2560               0 (served by _ws)
    atomic                   any: rows unsorted or a row index out of range          1
    per class: both sides of each threshold; vector counts 1, 5, J - 1, J, J + 1 with 1 and 3 batches; rows of 0, 1, R - 1, R, R + 1, 2R + 3 entries
    (R = the entries per round: 32 / 64 / 128 for J = 32 / 16 / 8, packed: the 32-entry pad unit), first and last row empty, a run of empty rows,
    37..70 rows (no multiple of 8); orders sorted / columns shuffled inside rows / shuffled / duplicates; columns out of range skipped in place
    row split (gridDim.y)    A_rows 511, 512, 520, 1030 -> 1, 2, 2, 4; 1025 (pk_scan_kernel: runs of 2 rows, most threads none)
    packed routing           A_nnz == 0, a workspace one byte short, one smaller than the row-pointer form's, a base that is not 16-byte aligned"""
import collections
import ctypes

import numpy as np
import pytest

from guard_testlib import Guarded, Workspace, canon32 as canon, margin_report_fixture, seed
from parity_testlib import FP32_TOL, bits, check_close, rand

pytestmark = pytest.mark.gpu

QNAN = np.uint32(0x7FC00000)
SENT = np.uint32(0x5A5A5A5A)
ALL1 = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = 64                     # words in front of and behind every buffer (a multiple of 16 bytes: the base alignment is the offset's)
INVALID, NOT_SUPPORTED = 1, 2
KINDS = ("ties", "uniform")
ABS = ((1.0, 0.0), (0.5, -2.0))
BATCH = 3


# ---------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------
def _seed(*xs):
    return seed(0x5718, *xs)


def Buf(payload, guard, off=0):
    """An input (4- or 8-byte elements, kept as bits) between GUARD guard words, `off` more of them in front."""
    return Guarded.around(payload, guard, GUARD + off, GUARD)


class CBuf(Guarded):
    """One allocation of sentinel words that holds the logical Cs (bit patterns): C_b for b in `order`, one after the other, GUARD words in front
    of the first and GUARD + 4 * (i + 1) behind the i-th -- unequal gaps; `off` shifts every base."""

    def __init__(self, payloads, off=0, order=None):
        order = list(range(len(payloads))) if order is None else list(order)
        assert sorted(order) == list(range(len(payloads)))
        self.start, self.sizes = [0] * len(payloads), [p.size for p in payloads]
        pos = GUARD + off
        for i, b in enumerate(order):
            self.start[b] = pos
            pos += payloads[b].size + GUARD + 4 * (i + 1)
        Guarded.__init__(self, pos, SENT, np.uint32, GUARD + off, np.concatenate([np.arange(s, s + n) for s, n in zip(self.start, self.sizes)]))
        for b, p in enumerate(payloads):
            self.host[self.start[b]:self.start[b] + p.size] = p

    def ptr(self, b=0):
        return self.dev.data_ptr() + 4 * self.start[b]

    def results(self, what):
        """The logical Cs as bits, after asserting that every sentinel around them kept its bits."""
        got = self.assert_outside_kept(lambda n, first: f"{what}: {n} words outside C were written, first at {first} (the Cs start at {self.start})")
        return [got[s:s + n] for s, n in zip(self.start, self.sizes)]


def compare(got_bits, ref, scale, kind, k, what, shape):
    """All of C against the fp64 reference: `ties` exactly (the reference converted to fp32), `uniform` through check_close."""
    g = got_bits.view(np.float32)
    bad = np.flatnonzero(np.isnan(g))
    assert bad.size == 0, f"{what}: {bad.size} NaN results (a guard or an empty block read into a product?), first at {np.unravel_index(bad[:4], shape)}"
    if kind == "ties":
        wrong = np.flatnonzero(g != ref.astype(np.float32))
        assert wrong.size == 0, (f"{what}: {wrong.size} of {g.size} results are not the exact product, first at {np.unravel_index(wrong[:4], shape)}: "
                                 f"{g[wrong[:4]]} for {ref[wrong[:4]]}")
    else:
        check_close(g, ref, scale, FP32_TOL, what, k, "f32")


def assert_ties_premise(ref, scale):
    assert scale.max() < 2.0 ** 24 and np.array_equal(np.rint(2.0 * ref), 2.0 * ref) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)


# ---------------------------------------------------------------------------------------------
# Blocked-ELL: cases
# ---------------------------------------------------------------------------------------------
BELL_ENTRIES = ("gather", "ws", "batched")
# route / gemm: the launch classes the case is named for (None: a structure case, named for none); nblk: stored blocks per block row
BellCase = collections.namedtuple("BellCase", "name rows cols bs nblk n pattern route gemm b_off c_off ws_off entries",
                                  defaults=("asc", None, None, 0, 0, 0, BELL_ENTRIES))
PATTERNS = ("asc", "desc", "shuf", "empties")

BELL_STRUCTURE = [
    BellCase("bs1", 40, 48, 1, 12, 8),
    BellCase("bs2-desc", 40, 48, 2, 8, 9, "desc"),
    BellCase("bs3-shuf-ragged", 41, 50, 3, 5, 1, "shuf"),              # 41 % 3 == 2: 14 block rows; 50 % 3 != 0: 16 block columns
    BellCase("bs4-empties-ragged", 42, 50, 4, 6, 8, "empties"),
    BellCase("bs8-empties-ragged", 44, 100, 8, 4, 9, "empties"),
    BellCase("bs2-empties", 40, 48, 2, 9, 9, "empties"),
    BellCase("ell0", 40, 48, 2, 0, 9),
    BellCase("ell0-scatter", 6, 12320, 4, 0, 8, route="scatter", gemm="dma<64,64>"),
    BellCase("rows255", 255, 48, 2, 6, 9, "shuf"),
    BellCase("rows256", 256, 48, 2, 6, 9, "shuf"),
    BellCase("rows257", 257, 48, 2, 6, 9, "shuf"),                      # ragged last block row in the second 256-row workgroup of the gather kernel
]
BELL_EXPANSION = [
    BellCase("cols12288", 40, 12288, 4, 8, 8, "shuf", "expand-vec", "dma<64,64>"),
    BellCase("cols12320", 24, 12320, 4, 8, 8, "empties", "scatter", "dma<64,64>"),
    BellCase("cols12292", 6, 12292, 2, 8, 9, "shuf", "scatter", "generic<64,64>"),
    BellCase("cols50", 40, 50, 2, 8, 9, "empties", "expand-elem", "generic<64,64>"),
    BellCase("ws+4", 40, 64, 2, 8, 40, "empties", "expand-elem", "generic<64,64>", ws_off=4, entries=("gather", "ws")),
]
_DMA_SHAPES = [("dma<64,64>", 40, 40), ("dma<64,128>", 40, 200), ("dma<128,64>", 72, 104), ("dma<128,128>", 72, 200)]   # (class, n, rows)
BELL_DISPATCH = [BellCase(f"{cls}-cols{cols}", rows, cols, 2, cols // 4, n, PATTERNS[(i + j) % 4], "expand-vec", cls)
                 for i, (cls, n, rows) in enumerate(_DMA_SHAPES) for j, cols in enumerate((64, 32, 160))]
BELL_DISPATCH += [
    BellCase("generic-cols72", 40, 72, 2, 18, 40, "shuf", "expand-vec", "generic<64,64>"),
    BellCase("generic-b_off1", 40, 64, 2, 16, 40, "empties", "expand-vec", "generic<64,64>", b_off=1),
    # both sides of the thresholds: n 64 / 68 (at rows <= 64 and at rows > 128), rows 64 / 68 (n <= 64), rows 128 / 132 (n > 64)
    BellCase("n64-rows40", 40, 64, 4, 8, 64, "asc", "expand-vec", "dma<64,64>"),
    BellCase("n68-rows40", 40, 64, 4, 8, 68, "asc", "expand-vec", "dma<128,64>"),
    BellCase("n64-rows200", 200, 64, 4, 8, 64, "desc", "expand-vec", "dma<64,128>"),
    BellCase("n68-rows200", 200, 64, 4, 8, 68, "desc", "expand-vec", "dma<128,128>"),
    BellCase("rows64-n40", 64, 64, 4, 8, 40, "shuf", "expand-vec", "dma<64,64>"),
    BellCase("rows68-n40", 68, 64, 4, 8, 40, "shuf", "expand-vec", "dma<64,128>"),
    BellCase("rows128-n72", 128, 64, 4, 8, 72, "empties", "expand-vec", "dma<128,64>"),
    BellCase("rows132-n72", 132, 64, 4, 8, 72, "empties", "expand-vec", "dma<128,128>"),
    # store branches: C + one float and odd rows (ldc % 4 != 0) store per element; the aligned C with rows % 4 == 0 is every case above
    BellCase("dma-c_off1", 40, 64, 2, 16, 40, "shuf", "expand-vec", "dma<64,64>", c_off=1),
    BellCase("dma-rows41", 41, 64, 2, 16, 40, "shuf", "expand-vec", "dma<64,64>"),
    BellCase("dma128-rows201-c_off1", 201, 64, 2, 16, 72, "asc", "expand-vec", "dma<128,128>", c_off=1),
    BellCase("generic-c_off1", 40, 72, 2, 18, 40, "desc", "expand-vec", "generic<64,64>", c_off=1),
    BellCase("generic-rows41", 41, 72, 2, 18, 40, "asc", "expand-vec", "generic<64,64>"),
]
BELL_CASES = BELL_STRUCTURE + BELL_EXPANSION + BELL_DISPATCH


def bell_blocks(rng, rows, cols, bs, nblk, pattern):
    """column_indices [ceil(rows / bs)][nblk]: distinct block columns per block row in the pattern's order.  `empties`: shuffled, with an empty
    block in the middle and one at the end of every block row -- marked ~0 and cols / bs, the two markers swapping places from one block row to
    the next -- and every fifth block row empty throughout."""
    nbr, nbc = -(-rows // bs), cols // bs
    assert nblk <= nbc and (pattern != "empties" or nblk >= 3)
    ci = np.argsort(rng.random((nbr, max(nbc, 1))), axis=1)[:, :nblk].astype(np.uint64)      # distinct per block row, shuffled
    if pattern in ("asc", "desc"):
        ci = np.sort(ci, axis=1)[:, ::1 if pattern == "asc" else -1]
    if pattern == "empties":
        even = np.arange(nbr) % 2 == 0
        mid, end = np.where(even, ALL1, np.uint64(nbc)), np.where(even, np.uint64(nbc), ALL1)
        ci[:, nblk // 2], ci[:, nblk - 1] = mid, end
        ci[4::5, :] = mid[4::5, None]
    return np.ascontiguousarray(ci)


class BellProblem:
    """One case and data kind: `batch` matrices (column_indices, values, C0) over one shared B, the references, and the inputs on the device."""

    def __init__(self, case, kind, batch=BATCH, seed_extra=()):
        self.case, self.kind, self.batch = case, kind, batch
        c = case
        self.ell_cols, self.nbc = c.nblk * c.bs, c.cols // c.bs
        rng = np.random.default_rng(_seed("bell", c.name, kind, *seed_extra))
        self.B = rand(rng, c.n * c.cols, np.float32, kind)
        self.ci, self.vals, self.C0 = [], [], []
        br = np.arange(c.rows) // c.bs
        for _ in range(batch):
            ci = bell_blocks(rng, c.rows, c.cols, c.bs, c.nblk, c.pattern)
            vals = rand(rng, c.rows * self.ell_cols, np.float32, kind).reshape(c.rows, self.ell_cols)
            for e in range(c.nblk):
                vals[ci[br, e] >= self.nbc, e * c.bs:(e + 1) * c.bs] = np.nan       # nothing may read the values of an empty block
            self.ci.append(ci)
            self.vals.append(vals)
            self.C0.append(rand(rng, c.n * c.rows, np.float32, kind))
        self._dense, self._refs = {}, {}

    def dense(self, b):
        """(A [rows][cols] in fp64, the longest row's term count) from the definition."""
        if b not in self._dense:
            c = self.case
            A = np.zeros((c.rows, c.cols))
            br = np.arange(c.rows) // c.bs
            terms = np.zeros(c.rows, dtype=np.int64)
            for e in range(c.nblk):
                bc = self.ci[b][br, e]
                ok = np.flatnonzero(bc < self.nbc)
                terms[ok] += c.bs
                for t in range(c.bs):
                    A[ok, bc[ok].astype(np.int64) * c.bs + t] = self.vals[b][ok, e * c.bs + t]
            assert not np.isnan(A).any()
            self._dense[b] = (A, int(terms.max()) if c.rows else 0)
        return self._dense[b]

    def reference(self, b, ab):
        """(ref, scale), [n][rows] flattened: alpha * A B + beta * C0 (C0 unread when beta == 0) and |alpha| |A| |B| + |beta| |C0|."""
        if (b, ab) not in self._refs:
            c = self.case
            A, _ = self.dense(b)
            Bm = self.B.astype(np.float64).reshape(c.n, c.cols)
            ref, scale = ab[0] * (Bm @ A.T), abs(ab[0]) * (np.abs(Bm) @ np.abs(A).T)
            if ab[1] != 0.0:
                c0 = self.C0[b].astype(np.float64).reshape(c.n, c.rows)
                ref, scale = ref + ab[1] * c0, scale + abs(ab[1]) * np.abs(c0)
            self._refs[(b, ab)] = ((ref + 0.0).reshape(-1), scale.reshape(-1))
        return self._refs[(b, ab)]

    def to_device(self):
        self.dV = [Buf(v, QNAN).to_device() for v in self.vals]
        self.dI = [Buf(ci, ALL1).to_device() for ci in self.ci]
        self.dB = Buf(self.B, QNAN, off=self.case.b_off).to_device()
        return self

    def inputs_unchanged(self):
        return all(x.unchanged() for x in self.dV + self.dI + [self.dB])


def call_bell(L, entry, c, ell_cols, V, I, B, C, ab, ws=0, batch=BATCH, n=None):
    """The status of one call; V, I, C: pointers (batched: ctypes arrays of them), as integers so that the refusals run without a device."""
    n = c.n if n is None else n
    if entry == "gather":
        return L.sm_spmm_bell_f32(V, I, c.rows, c.cols, c.bs, ell_cols, B, C, n, ab[0], ab[1], None)
    if entry == "ws":
        return L.sm_spmm_bell_f32_ws(V, I, c.rows, c.cols, c.bs, ell_cols, B, C, n, ab[0], ab[1], ws, None)
    assert entry == "batched"
    return L.sm_spmm_bell_batched_f32(V, I, c.rows, c.cols, c.bs, ell_cols, B, C, n, batch, ab[0], ab[1], ws, None)


def run_bell(gpu, p, entry, ab, what):
    """One entry point on the problem's device inputs and a fresh guarded C; every check of the docstring; the Cs as bits."""
    L, c = gpu.lib(), p.case
    nb = p.batch if entry == "batched" else 1
    c0 = [bits(p.C0[b]) if ab[1] != 0.0 else np.full(c.n * c.rows, QNAN, dtype=np.uint32) for b in range(nb)]
    order = np.random.default_rng(_seed("order", c.name)).permutation(nb)
    C = CBuf(c0, off=c.c_off, order=order).to_device()
    need, ws = ctypes.c_size_t(0), None
    if entry == "gather":
        rc = call_bell(L, entry, c, p.ell_cols, p.dV[0].ptr, p.dI[0].ptr, p.dB.ptr, C.ptr(0), ab)
    elif entry == "ws":
        assert L.sm_spmm_bell_workspace_size(c.rows, c.cols, ctypes.byref(need)) == 0
        ws = Workspace(need.value, c.ws_off)
        rc = call_bell(L, entry, c, p.ell_cols, p.dV[0].ptr, p.dI[0].ptr, p.dB.ptr, C.ptr(0), ab, ws.ptr)
    else:
        assert L.sm_spmm_bell_batched_workspace_size(c.rows, c.cols, nb, ctypes.byref(need)) == 0
        ws = Workspace(need.value, c.ws_off)
        Arr = ctypes.c_void_p * nb
        rc = call_bell(L, entry, c, p.ell_cols, Arr(*[v.ptr for v in p.dV]), Arr(*[i.ptr for i in p.dI]), p.dB.ptr, Arr(*[C.ptr(b) for b in range(nb)]), ab,
                       ws.ptr, nb)
    assert rc == 0, f"{what}: status {rc}: {L.sm_last_error().decode()}"
    got = C.results(what)
    if ws is not None:
        ws.check(what)
    assert p.inputs_unchanged(), f"{what}: an input or one of its guards was modified"
    for b in range(nb):
        ref, scale = p.reference(b, ab)
        compare(got[b], ref, scale, p.kind, p.dense(b)[1] + 2, f"{what} batch {b}" if nb > 1 else what, (c.n, c.rows))
    return got


def bell_runs(p):
    """(entry, (alpha, beta)) of one problem: `ties` with both pairs, `uniform` with one (the other one on every second case)."""
    i = [c.name for c in BELL_CASES].index(p.case.name) if p.case in BELL_CASES else 0
    for ab in (ABS if p.kind == "ties" else (ABS[i % 2],)):
        for entry in p.case.entries:
            yield entry, ab


@pytest.mark.parametrize("case", BELL_CASES, ids=lambda c: c.name)
def test_bell_on_guarded_operands(gpu, case):
    for kind in KINDS:
        p = BellProblem(case, kind)
        if kind == "ties":
            for b in range(p.batch):
                for ab in ABS:
                    assert_ties_premise(*p.reference(b, ab))
        p.to_device()
        for entry, ab in bell_runs(p):
            run_bell(gpu, p, entry, ab, f"sm_spmm_bell[{entry}] {kind} {case.name} ab {ab}")


# ---- the register-staged GEMM's 128 x 64 tiling: from 32 64 x 64 tiles per CU on; only the batched form brings that many at a small size
BIG_BATCH = 64


def big_generic_shape(cus):
    """(rows, cols, n, batch): one 64-wide tile along n, ceil(rows / 64) * batch >= 32 * cus tiles, rows no multiple of 64, cols % 32 != 0."""
    return -(-32 * cus // BIG_BATCH) * 64 - 24, 24, 5, BIG_BATCH


@pytest.mark.parametrize("kind", KINDS)
def test_bell_generic_128x64_tiles(gpu, kind):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, cols, n, batch = big_generic_shape(cus)
    assert -(-n // 64) * -(-rows // 64) * batch >= 32 * cus and cols % 32 != 0, "the case does not reach launch32<128, 64, 4, 1, 2>"
    case = BellCase("big-generic", rows, cols, 4, 4, n, "empties", "expand-vec", "generic<128,64>", entries=("batched",))
    p = BellProblem(case, kind, batch=batch, seed_extra=(cus,))
    ab = ABS[1]
    if kind == "ties":
        for b in range(batch):
            assert_ties_premise(*p.reference(b, ab))
    run_bell(gpu, p.to_device(), "batched", ab, f"sm_spmm_bell[batched] {kind} generic<128,64> (rows, cols, n, batch) = {(rows, cols, n, batch)}")


# ---------------------------------------------------------------------------------------------
# COO: cases
# ---------------------------------------------------------------------------------------------
COO_ENTRIES = ("plain", "ws", "packed")
COO_CLASSES = ("ws J32", "ws J16", "ws J8", "ws row", "packed J32", "packed J16", "packed->ws")
ROUND_ENTRIES = {"ws J32": 32, "ws J16": 64, "ws J8": 128, "ws row": 32, "packed J32": 32, "packed J16": 32, "packed->ws": 128}   # R of the row lengths
GROUP = {"ws J32": 32, "ws J16": 16, "ws J8": 8, "ws row": 16, "packed J32": 32, "packed J16": 16, "packed->ws": 8}   # vectors per workgroup (ws row: columns)
# matrix: "lens" (rows of 0, 1, R - 1, R, R + 1, 2R + 3, 0, 0, 0, 5 entries, in turn; first and last row empty) or "split" (see coo_lengths)
# order: sorted / colshuf / shuffled / dups; oob: None / "col" / "rowhi" / "rowneg"
CooCase = collections.namedtuple("CooCase", "name cls m k n batches matrix order oob", defaults=("lens", "sorted", None))


def entry_of(cls):
    return cls.split()[0].split("-")[0]


def expected_flag(case):
    """The first int of the workspace after the call: 1 when the rows are unsorted or one is out of range, else 4 for the packed kernel, else 0."""
    if case.order == "shuffled" or case.oob in ("rowhi", "rowneg"):
        return 1
    return 4 if case.cls in ("packed J32", "packed J16") else 0


def _nb(nv):
    """(B_num_cols, num_batches) with that many vectors: three batches where nv allows."""
    return (nv // 3, 3) if nv % 3 == 0 and nv > 3 else (nv, 1)


THRESHOLD_COLS = {"ws J32": (576,), "ws J16": (577, 2304), "ws J8": (2305, 4608), "ws row": (4609,), "packed J32": (639,), "packed J16": (640, 2559),
                  "packed->ws": (2560,)}
CLASS_COLS = {"ws J32": 70, "ws J16": 600, "ws J8": 2400, "ws row": 4700, "packed J32": 70, "packed J16": 700, "packed->ws": 2600}
_ROWS = (37, 39, 41, 43, 45, 47, 49, 51, 53, 55, 57, 59, 61, 62, 66, 67, 69, 70)      # 37..70, no multiple of 8


def _coo_cases():
    out, i = [], 0

    def rows():
        nonlocal i
        i += 1
        return _ROWS[i % len(_ROWS)]
    for cls, ks in THRESHOLD_COLS.items():      # both sides of every threshold, the last vector group ragged
        for k in ks:
            out.append(CooCase(f"{cls}-cols{k}", cls, rows(), k, *_nb(GROUP[cls] + 1)))
    for cls, k in CLASS_COLS.items():
        J = GROUP[cls]
        for nv in (1, 5, J - 1, J, J + 1):      # (ws row: its groups are CSR_J = 16 columns of ONE batch: B_num_cols takes these values)
            n, b = (nv, 3 if nv in (5, J) else 1) if cls == "ws row" else _nb(nv)
            out.append(CooCase(f"{cls}-nv{nv}", cls, rows(), k, n, b))
        for order in ("colshuf", "shuffled", "dups"):
            out.append(CooCase(f"{cls}-{order}", cls, rows(), k, 5, 1, "lens", order))
        out.append(CooCase(f"{cls}-oobcol", cls, rows(), k, 5, 1, "lens", "colshuf", "col"))
    for cls in ("ws J32", "packed J32"):
        for oob in ("rowhi", "rowneg"):
            out.append(CooCase(f"{cls}-{oob}", cls, rows(), 70, 5, 1, "lens", "sorted", oob))
        for m in (511, 512, 520, 1030) + ((1025,) if cls == "packed J32" else ()):
            out.append(CooCase(f"{cls}-rows{m}", cls, m, 40, 5, 1, "split"))
        out.append(CooCase(f"{cls}-rows1030-dups", cls, 1030, 40, 2, 3, "split", "dups", "col"))
    return out


COO_CASES = _coo_cases()


def row_split(m, groups):
    """gridDim.y of the LDS-CSR and the packed kernel (launch_csr_lds, launch_csr_packed)."""
    s = 1
    while groups * s < 1024 and m // (s * 2) >= 256:
        s *= 2
    return s


def coo_lengths(rng, case):
    R, m = ROUND_ENTRIES[case.cls], case.m
    if case.matrix == "lens":
        cyc = (0, 1, R - 1, R, R + 1, 2 * R + 3, 0, 0, 0, 5)
        lens = np.array([cyc[i % 10] for i in range(m)])
    else:   # "split": 0..12 entries per row, a run of empty rows, and per split of the rows an empty first row and a non-zero in the last
        lens = rng.integers(0, 13, m)
        lens[100:110] = 0
        s = row_split(m, 1)
        per = -(-m // s)
        for y in range(s):
            lens[y * per] = 0
            lens[min((y + 1) * per, m) - 1] = 1 + y
        lens[m - 1] = 7                  # (the last row of the last split; the lens matrices have it empty)
        return lens
    lens[0] = lens[m - 1] = 0
    return lens


def coo_entries(rng, case):
    """(rows, cols) int32 in the case's order."""
    m, k = case.m, case.k
    lens = coo_lengths(rng, case)
    assert lens.max() <= k
    r = np.repeat(np.arange(m), lens).astype(np.int32)
    c = np.concatenate([np.sort(rng.permutation(k)[:n_]) for n_ in lens]).astype(np.int32)
    if case.order == "colshuf":
        c = np.concatenate([rng.permutation(c[r == i]) for i in range(m)]).astype(np.int32)
    elif case.order == "dups":          # a tenth of the entries once more, behind their row's own (rows sorted, columns not)
        idx = rng.choice(r.size, max(3, r.size // 10), replace=False)
        r, c = np.concatenate([r, r[idx]]), np.concatenate([c, c[idx]])
        o = np.argsort(r, kind="stable")
        r, c = r[o], c[o]
    elif case.order == "shuffled":
        o = rng.permutation(r.size)
        r, c = r[o], c[o]
    if case.oob == "col":               # skipped in place: the rows stay sorted
        idx = rng.choice(r.size, 6, replace=False)
        c[idx] = np.array([-1, -7, k, k + 9, 2 ** 31 - 1, -2 ** 31], dtype=np.int64).astype(np.int32)
    elif case.oob == "rowhi":           # still ascending: only the range check sends the call to the atomic kernel
        r[-1] = m
    elif case.oob == "rowneg":
        r[0] = -1
    return np.ascontiguousarray(r), np.ascontiguousarray(c)


class CooProblem:
    def __init__(self, case, kind, entries=None):
        self.case, self.kind = case, kind
        rng = np.random.default_rng(_seed("coo", case.name, kind))
        self.r, self.c = coo_entries(rng, case) if entries is None else entries
        self.nnz, self.nv = self.r.size, case.n * case.batches
        self.v = rand(rng, self.nnz, np.float32, kind)
        self.B = rand(rng, self.nv * case.k, np.float32, kind)
        self.C0 = rand(rng, self.nv * case.m, np.float32, kind)
        self._refs = {}

    def valid(self):
        r, c = self.r.astype(np.int64), self.c.astype(np.int64)
        return (r >= 0) & (r < self.case.m) & (c >= 0) & (c < self.case.k)

    def terms(self):
        ok = self.valid()
        return int(np.bincount(self.r[ok], minlength=self.case.m).max()) if ok.any() else 0

    def reference(self, ab):
        """(ref, scale), [vector][row] flattened (vector = batch * B_num_cols + column: the batch strides are exactly one matrix)."""
        if ab not in self._refs:
            m, k = self.case.m, self.case.k
            ok = self.valid()
            A, absA = np.zeros((m, k)), np.zeros((m, k))
            np.add.at(A, (self.r[ok], self.c[ok]), self.v[ok].astype(np.float64))
            np.add.at(absA, (self.r[ok], self.c[ok]), np.abs(self.v[ok].astype(np.float64)))
            V = self.B.astype(np.float64).reshape(self.nv, k)
            ref, scale = ab[0] * (V @ A.T), abs(ab[0]) * (np.abs(V) @ absA.T)
            if ab[1] != 0.0:
                c0 = self.C0.astype(np.float64).reshape(self.nv, m)
                ref, scale = ref + ab[1] * c0, scale + abs(ab[1]) * np.abs(c0)
            self._refs[ab] = ((ref + 0.0).reshape(-1), scale.reshape(-1))
        return self._refs[ab]

    def to_device(self):
        zero = np.uint32(0)
        self.dR, self.dC, self.dV = Buf(self.r, zero).to_device(), Buf(self.c, zero).to_device(), Buf(self.v, QNAN).to_device()
        self.dB = Buf(self.B, QNAN).to_device()
        return self

    def inputs_unchanged(self):
        return all(x.unchanged() for x in (self.dR, self.dC, self.dV, self.dB))


def pk_bytes(m, nnz):
    """The bytes the packed form needs (pk_plan: flag, row pointers, padded row offsets, the entry stream and its slack), before rounding to 256."""
    o = (2 * m + 3 + 3) // 4 * 4
    return 4 * (o + 2 * (nnz + 31 * m + 6 * 32))


def call_coo(L, entry, c, nnz, R, Cc, V, B, C, ab, ws=0, ws_bytes=0, n=None, batches=None, m=None):
    n, batches, m = c.n if n is None else n, c.batches if batches is None else batches, c.m if m is None else m
    if entry == "plain":
        return L.sm_spmm_coo_f32(m, c.k, nnz, n, batches, R, Cc, V, B, C, ab[0], ab[1], None)
    if entry == "ws":
        return L.sm_spmm_coo_f32_ws(m, c.k, nnz, n, batches, R, Cc, V, B, C, ab[0], ab[1], ws, None)
    assert entry == "packed"
    return L.sm_spmm_coo_f32_packed(m, c.k, nnz, n, batches, R, Cc, V, B, C, ab[0], ab[1], ws, ws_bytes, None)


def coo_workspace(L, entry, c, nnz):
    need = ctypes.c_size_t(0)
    if entry == "ws":
        assert L.sm_spmm_coo_workspace_size(c.m, ctypes.byref(need)) == 0
    else:
        assert L.sm_spmm_coo_packed_workspace_size(c.m, nnz, ctypes.byref(need)) == 0
    return need.value


def run_coo(gpu, p, entry, ab, what, flag=None, ws_bytes=None, ws_off=0, untouched=False, check=True):
    """One entry point on the problem's device inputs and a fresh guarded C; the workspace has the reported size (or ws_bytes); C as bits."""
    L, c = gpu.lib(), p.case
    C = CBuf([bits(p.C0) if ab[1] != 0.0 else np.full(p.nv * c.m, QNAN, dtype=np.uint32)]).to_device()
    ws = None
    if entry != "plain":
        nbytes = coo_workspace(L, entry, c, p.nnz) if ws_bytes is None else ws_bytes
        ws = Workspace(nbytes, ws_off)
    rc = call_coo(L, entry, c, p.nnz, p.dR.ptr, p.dC.ptr, p.dV.ptr, p.dB.ptr, C.ptr(0), ab, ws.ptr if ws else 0, ws.nbytes if ws else 0)
    assert rc == 0, f"{what}: status {rc}: {L.sm_last_error().decode()}"
    got = C.results(what)[0]
    if ws is not None:
        ws.check(what, untouched)
        if flag is not None:
            assert ws.flag() == flag, f"{what}: flag word {ws.flag()}, not {flag}: the call did not run the class it is named for"
    assert p.inputs_unchanged(), f"{what}: an input or one of its guards was modified"
    if check:
        ref, scale = p.reference(ab)
        compare(got, ref, scale, p.kind, p.terms() + 2, what, (p.nv, c.m))
    return got


@pytest.mark.parametrize("case", COO_CASES, ids=lambda c: c.name)
def test_coo_on_guarded_operands(gpu, case):
    entry = entry_of(case.cls)
    i = COO_CASES.index(case)
    for kind in KINDS:
        p = CooProblem(case, kind)
        if kind == "ties":
            for ab in ABS:
                assert_ties_premise(*p.reference(ab))
        p.to_device()
        for ab in (ABS if kind == "ties" else (ABS[i % 2],)):
            got = run_coo(gpu, p, entry, ab, f"sm_spmm_coo[{entry}] {kind} {case.name} ab {ab}", flag=expected_flag(case))
            if kind == "ties":      # exact in any order: the three entry points agree bit for bit
                for other in COO_ENTRIES:
                    if other != entry:
                        same = run_coo(gpu, p, other, ab, f"sm_spmm_coo[{other}] {kind} {case.name} ab {ab}")
                        assert np.array_equal(canon(same), canon(got)), f"{case.name}: {other} and {entry} differ on integer data"


@pytest.mark.parametrize("case", [c for c in COO_CASES if c.order in ("sorted", "colshuf", "dups") and c.oob in (None, "col")
                                  and (c.name.endswith(("-nv5", "-colshuf", "-dups", "-oobcol")) or c.matrix == "split")], ids=lambda c: c.name)
def test_coo_sorted_rows_give_the_same_bits_on_every_call(gpu, case):
    entry = entry_of(case.cls)
    p = CooProblem(case, "uniform").to_device()
    what = f"sm_spmm_coo[{entry}] reproducible {case.name}"
    first = run_coo(gpu, p, entry, ABS[1], what, flag=expected_flag(case))
    again = run_coo(gpu, p, entry, ABS[1], what, flag=expected_flag(case), check=False)
    assert np.array_equal(first, again), f"{what}: two calls on row-sorted input differ"


# ---- the packed entry point's own routing: each must give what sm_spmm_coo_f32 gives
PACKED_ROUTING = ("nnz0", "one-byte-short", "below-rowptr", "unaligned")
ROUTING_CASE = CooCase("packed-routing", "packed J32", 53, 70, 11, 3)


def routing_setup(mode, kind, L_sizes=None):
    """(problem, workspace bytes, workspace offset, flag word or None, whether the workspace stays untouched)."""
    case = ROUTING_CASE
    if mode == "nnz0":
        p = CooProblem(case, kind, entries=(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)))
        return p, None, 0, 0, False
    p = CooProblem(case, kind)
    if mode == "one-byte-short":
        return p, pk_bytes(case.m, p.nnz) - 1, 0, 0, False
    if mode == "below-rowptr":
        return p, 4 * (case.m + 2) - 1, 0, None, True
    assert mode == "unaligned"
    return p, None, 4, 0, False


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", PACKED_ROUTING)
def test_coo_packed_routing(gpu, mode, kind):
    p, ws_bytes, ws_off, flag, untouched = routing_setup(mode, kind)
    p.to_device()
    for ab in ABS:
        what = f"sm_spmm_coo[packed] {mode} {kind} ab {ab}"
        got = run_coo(gpu, p, "packed", ab, what, flag=flag, ws_bytes=ws_bytes, ws_off=ws_off, untouched=untouched)
        if kind == "ties":
            assert_ties_premise(*p.reference(ab))
            plain = run_coo(gpu, p, "plain", ab, what + " (sm_spmm_coo_f32)")
            assert np.array_equal(canon(got), canon(plain)), f"{what}: differs from sm_spmm_coo_f32"
        if mode in ("nnz0", "below-rowptr"):     # beta * C0 on the empty rows, bit for bit (zeros when beta == 0)
            ok = p.valid()
            empty = np.setdiff1d(np.arange(p.case.m), p.r[ok])
            want = np.float32(ab[1]) * p.C0.reshape(p.nv, p.case.m)[:, empty] if ab[1] != 0.0 else np.zeros((p.nv, empty.size), dtype=np.float32)
            assert empty.size and np.array_equal(got.view(np.float32).reshape(p.nv, p.case.m)[:, empty], want), f"{what}: an empty row is not beta * C0"


# ---------------------------------------------------------------------------------------------
# refusals: decided before any device call (tests/test_spmm32_cases.py calls them with dummy pointers); here: C stays untouched
# ---------------------------------------------------------------------------------------------
BIG = 2 ** 31
# name -> (family, entry, what differs from a valid call, status)
REFUSALS = {
    "bell null values": ("bell", BELL_ENTRIES, dict(V=0), INVALID),
    "bell null indices": ("bell", BELL_ENTRIES, dict(I=0), INVALID),
    "bell null B": ("bell", BELL_ENTRIES, dict(B=0), INVALID),
    "bell null C": ("bell", BELL_ENTRIES, dict(C=0), INVALID),
    "bell block_size 0": ("bell", BELL_ENTRIES, dict(bs=0), INVALID),
    "bell ell_cols % block_size": ("bell", BELL_ENTRIES, dict(ell_cols=7), INVALID),
    "bell batched without a workspace": ("bell", ("batched",), dict(ws=0), INVALID),
    "bell gather n > 8 * 65535": ("bell", ("gather",), dict(n=8 * 65535 + 1), NOT_SUPPORTED),
    "bell rows > 2^31-1": ("bell", ("ws", "batched"), dict(rows=BIG), NOT_SUPPORTED),
    "bell cols > 2^31-1": ("bell", ("ws", "batched"), dict(cols=BIG), NOT_SUPPORTED),
    "bell n > 2^31-1": ("bell", ("ws", "batched"), dict(n=BIG), NOT_SUPPORTED),
    "bell batch > 65535": ("bell", ("batched",), dict(batch=65536), NOT_SUPPORTED),
    "coo null B": ("coo", COO_ENTRIES, dict(B=0), INVALID),
    "coo null C": ("coo", COO_ENTRIES, dict(C=0), INVALID),
    "coo null rows": ("coo", COO_ENTRIES, dict(R=0), INVALID),
    "coo null cols": ("coo", COO_ENTRIES, dict(Cc=0), INVALID),
    "coo null vals": ("coo", COO_ENTRIES, dict(V=0), INVALID),
    "coo plain more than 65535 vectors": ("coo", ("plain",), dict(n=21846, batches=3), NOT_SUPPORTED),
    "coo ws nnz > 2^31-1": ("coo", ("ws",), dict(nnz=BIG), NOT_SUPPORTED),
    "coo ws batches > 65535": ("coo", ("ws",), dict(batches=65536), NOT_SUPPORTED),
    "coo ws B_num_cols > 16 * 65535": ("coo", ("ws",), dict(n=16 * 65535 + 1), NOT_SUPPORTED),
}
REFUSAL_BELL = BellCase("refusal", 40, 48, 4, 2, 9)
REFUSAL_COO = CooCase("refusal", "ws J32", 37, 70, 5, 1)


def call_refusal(L, name, V, I, B, C, ws, entry, nnz=100):
    """The status of REFUSALS[name] through `entry`; V: values / vals, I: column_indices / (rows, cols); pointers as integers."""
    fam, _, over, _ = REFUSALS[name]
    if fam == "bell":
        c = REFUSAL_BELL._replace(rows=over.get("rows", 40), cols=over.get("cols", 48), bs=over.get("bs", 4))
        batch = over.get("batch", BATCH)
        V, I, B, C, ws = (over.get(key, val) for key, val in (("V", V), ("I", I), ("B", B), ("C", C), ("ws", ws)))
        if entry == "batched":      # host tables of pointers (a null TABLE is the refusal; its entries are never read before the decision)
            Arr = ctypes.c_void_p * BATCH
            V, I, C = (Arr(*[x + 4096 * b for b in range(BATCH)]) if x else None for x in (V, I, C))
        return call_bell(L, entry, c, over.get("ell_cols", 8), V, I, B, C, ABS[1], ws, batch, over.get("n", 9))
    R, Cc = I
    R, Cc, V, B, C = (over.get(key, val) for key, val in (("R", R), ("Cc", Cc), ("V", V), ("B", B), ("C", C)))
    return call_coo(L, entry, REFUSAL_COO, over.get("nnz", nnz), R, Cc, V, B, C, ABS[1], ws, 1 << 40, over.get("n"), over.get("batches"))


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_c_alone(gpu, name):
    fam, entries, over, status = REFUSALS[name]
    L = gpu.lib()
    if fam == "bell":
        p = BellProblem(REFUSAL_BELL, "uniform").to_device()
        C = CBuf([bits(p.C0[b]) for b in range(BATCH)]).to_device()
        ws = Workspace(1 << 16)
        for entry in entries:
            if entry == "batched":
                Arr = ctypes.c_void_p * BATCH
                ov = {key: over[key] for key in ("V", "I", "C") if key in over}
                V, I, Cp = (None if key in ov else Arr(*ptrs) for key, ptrs in (("V", [v.ptr for v in p.dV]), ("I", [i.ptr for i in p.dI]),
                                                                                 ("C", [C.ptr(b) for b in range(BATCH)])))
                c = REFUSAL_BELL._replace(rows=over.get("rows", 40), cols=over.get("cols", 48), bs=over.get("bs", 4))
                rc = call_bell(L, entry, c, over.get("ell_cols", 8), V, I, over.get("B", p.dB.ptr), Cp, ABS[1], over.get("ws", ws.ptr), over.get("batch", BATCH),
                               over.get("n", 9))
            else:
                rc = call_refusal(L, name, p.dV[0].ptr, p.dI[0].ptr, p.dB.ptr, C.ptr(0), ws.ptr, entry)
            assert rc == status, f"{name} {entry}: status {rc}, not {status}"
            assert all(np.array_equal(g, bits(p.C0[b])) for b, g in enumerate(C.results(name))), f"{name} {entry}: a refused call wrote to C"
            ws.check(name, untouched=True)
    else:
        p = CooProblem(REFUSAL_COO, "uniform").to_device()
        C = CBuf([bits(p.C0)]).to_device()
        ws = Workspace(1 << 16)
        for entry in entries:
            rc = call_refusal(L, name, p.dV.ptr, (p.dR.ptr, p.dC.ptr), p.dB.ptr, C.ptr(0), ws.ptr, entry, nnz=p.nnz)
            assert rc == status, f"{name} {entry}: status {rc}, not {status}"
            assert np.array_equal(C.results(name)[0], bits(p.C0)), f"{name} {entry}: a refused call wrote to C"
            ws.check(name, untouched=True)


# ---------------------------------------------------------------------------------------------
# margins of this file's `uniform` comparisons, appended to the session's report: the worst per entry point, then the worst cases
# ---------------------------------------------------------------------------------------------
_spmm32_margin_report = margin_report_fixture(
    "{n} comparisons of tests/test_gpu_spmm32.py against the numpy fp64 product; err / bound (check_close), worst per entry point:", per_first_word=True)
