"""The dense 1-byte GEMM on the device (gemm_b8.hip): sm_gemm_rowmajor_fp8 and sm_gemm_rowmajor_i8[_q].  Exact products on
operands whose every fp32 partial sum is exact (and on integers), the dense form against the sparse one on the same pruned
matrix, the epilogue over every batch / shape case, specials, graph replay, the full-size ResNet-50 shapes and the driver."""
import os
import subprocess

import numpy as np
import pytest
# torch (and its HIP runtime) is loaded when the module is collected, before any test opens the product library: this file
# then runs on its own as well as in the whole suite
import torch  # noqa: F401

# (val64 here is torch's own conversion of the bytes: b8_testlib keeps it apart from the one through the fp16 image)
from b8_testlib import EXACT_VALS, FMTS, OUTS, PAIRS, ROUND, TINY, bytes_of, dev8, finite_bytes, ksteps, odt, tdt, to8, val64_direct as val64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(C):
    import torch
    return C.float().cpu().numpy().astype(np.float64) if C.dtype != torch.float32 else C.cpu().numpy().astype(np.float64)


def rounded(x, out):
    """fp64 values (exact in fp32) rounded once to the output type"""
    import torch
    return torch.from_numpy(x.astype(np.float32)).to(odt(out)).float().numpy().astype(np.float64)


def a_rows(a, m, k, lda, batch, strideA):
    """the logical [batch][m][k] A of a strided byte buffer"""
    return np.stack([np.stack([a[b * strideA + i * lda: b * strideA + i * lda + k] for i in range(m)]) for b in range(batch)])


def ref_fp8(A3, fa, bt, fb, n, k, batch, shared):
    """fp64 A_b . B_b and sum |a||b| per batch (A3: [batch][m][k] bytes, bt: [n][k] bytes per batch)"""
    A = val64(A3, fa)
    B = val64(bt, fb).reshape(1 if shared else batch, n, k)
    Bb = [B[0 if shared else i] for i in range(batch)]
    return np.stack([A[i] @ Bb[i].T for i in range(batch)]), np.stack([np.abs(A[i]) @ np.abs(Bb[i]).T for i in range(batch)])


def same_bits(x, y):
    import torch
    v = torch.int32 if x.dtype == torch.float32 else torch.int16
    return torch.equal(x.view(v), y.view(v))


# ---------------------------------------------------------------------------------------------
# exact products
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("out", OUTS)
def test_gemm_fp8_exact_products(gpu, fa, fb, out):
    """Values in {0, +-0.5, ..., +-4}: every product and fp32 partial sum is exact, so C is the fp64 product rounded once to
    the output type, bit for bit -- which holds only if A and B share the instruction's k-to-lane map, the format codes are
    right and the scale is 1.  B is random, so asymmetric: a row / column swap of C would show."""
    import torch
    rng = np.random.default_rng(11 + 7 * FMTS.index(fa) + 3 * FMTS.index(fb) + OUTS.index(out))
    for (m, n, k, batch) in [(64, 64, 128, 1), (130, 72, 192, 2), (33, 17, 256, 3), (2, 8, 64, 1), (258, 200, 320, 2)]:
        a = to8(rng.choice(EXACT_VALS, m * k * batch), fa)
        for shared in (True, False):
            bt = to8(rng.choice(EXACT_VALS, n * k * (1 if shared else batch)), fb)
            C = torch.full((batch * m * n,), 9.0, dtype=odt(out), device="cuda")
            gpu.gemm_rowmajor_fp8(dev8(a, fa), dev8(bt, fb), C, m, n, k, batch=batch, strideB=0 if shared else n * k)
            prod, _ = ref_fp8(a.reshape(batch, m, k), fa, bt, fb, n, k, batch, shared)
            want = torch.from_numpy(prod.astype(np.float32).reshape(-1)).to(odt(out)).cuda()
            assert same_bits(C, want), f"{fa} x {fb} -> {out} {(m, n, k, batch)} shared={shared}"


def test_gemm_fp8_identity_with_asymmetric_b(gpu):
    """A = I (m = k = 128): C row i is B's column i -- B[j][i] as stored [n][k] -- so C = B^T exactly, not B."""
    import torch
    m = k = 128
    n = 96
    rng = np.random.default_rng(5)
    eye = to8(np.eye(m, k, dtype=np.float32).reshape(-1), "e4m3")
    bt = to8(rng.choice(EXACT_VALS, n * k), "e4m3")
    C = torch.empty(m * n, dtype=torch.float32, device="cuda")
    gpu.gemm_rowmajor_fp8(dev8(eye, "e4m3"), dev8(bt, "e4m3"), C, m, n, k)
    assert np.array_equal(host(C).reshape(m, n), val64(bt, "e4m3").reshape(n, k).T)


def _i8_ref(a3, bt, n, k, batch, shared):
    B = bt.astype(np.int64).reshape(1 if shared else batch, n, k)
    return np.stack([a3[i].astype(np.int64) @ B[0 if shared else i].T for i in range(batch)])


@pytest.mark.parametrize("shape", [(64, 64, 128, 1), (130, 72, 192, 2), (33, 17, 256, 3), (2, 8, 64, 1), (258, 200, 1024, 2), (96, 40, 64, 2)])
def test_gemm_i8_exact(gpu, shape):
    """full int8 range (including -128 and 127, extremes forced into every row): C equals the int64 product; accumulate adds"""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + n + k + batch)
    a = rng.integers(-128, 128, (batch, m, k)).astype(np.int8)
    a[:, :, 0], a[:, :, -1] = -128, 127
    for shared in (True, False):
        bt = rng.integers(-128, 128, n * k * (1 if shared else batch)).astype(np.int8)
        bt[:k] = -128
        dA, dB = torch.from_numpy(a.reshape(-1)).cuda(), torch.from_numpy(bt).cuda()
        sB = 0 if shared else n * k
        want = _i8_ref(a, bt, n, k, batch, shared)
        C = torch.full((batch * m * n,), 12345, dtype=torch.int32, device="cuda")
        gpu.gemm_rowmajor_i8(dA, dB, C, m, n, k, batch=batch, strideB=sB)
        assert np.array_equal(C.cpu().numpy().astype(np.int64).reshape(want.shape), want), f"{shape} shared={shared}"
        c0 = rng.integers(-2 ** 20, 2 ** 20, batch * m * n).astype(np.int32)
        C = torch.from_numpy(c0).cuda()
        gpu.gemm_rowmajor_i8(dA, dB, C, m, n, k, batch=batch, strideB=sB, accumulate=True)
        assert np.array_equal(C.cpu().numpy().astype(np.int64).reshape(want.shape), want + c0.astype(np.int64).reshape(want.shape)), \
            f"{shape} shared={shared} accumulate"


@pytest.mark.parametrize("shape", [(64, 64, 128, 1), (130, 72, 192, 2), (33, 17, 256, 3), (128, 256, 512, 2)])
def test_gemm_i8_q_requantises_once(gpu, shape):
    """C = sat_int8(rint(float32(scale) * float32(acc))), bit for bit"""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(3 * m + n + k)
    a = rng.integers(-128, 128, (batch, m, k)).astype(np.int8)
    bt = rng.integers(-128, 128, n * k).astype(np.int8)
    acc = _i8_ref(a, bt, n, k, batch, True)
    for scale in (1.0 / 4096.0, 3.0e-4, 0.01, -2.5e-3):
        C = torch.full((batch * m * n,), 99, dtype=torch.int8, device="cuda")
        gpu.gemm_rowmajor_i8_q(torch.from_numpy(a.reshape(-1)).cuda(), torch.from_numpy(bt).cuda(), C, m, n, k, scale, batch=batch)
        want = np.clip(np.rint(np.float32(scale) * acc.astype(np.float32)), -128, 127).astype(np.int8)
        assert np.array_equal(C.cpu().numpy().reshape(want.shape), want), f"{shape} scale={scale}"


# ---------------------------------------------------------------------------------------------
# dense vs sparse on the same pruned matrix
# ---------------------------------------------------------------------------------------------
def _pruned_pair_fp8(gpu, a, fa, m, k, batch):
    """(blob, decompress24_fp8(blob)) of A pruned by compress24_fp8's STRIP rule"""
    import torch
    blob = torch.empty(gpu.compress24_size(m, k, 1, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24_fp8(dev8(a, fa), m, k, k, batch, m * k, blob)
    dense = dev8(np.zeros(batch * m * k, dtype=np.uint8), fa)
    gpu.decompress24_fp8(blob, m, k, k, batch, m * k, dense)
    return blob, dense


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("out", OUTS)
def test_gemm_fp8_vs_spmma_fp8_on_the_pruned_matrix(gpu, fa, fb, out):
    import torch
    rng = np.random.default_rng(500 + 7 * FMTS.index(fa) + 3 * FMTS.index(fb) + OUTS.index(out))
    for (m, n, k, batch) in [(196, 256, 512, 2), (130, 72, 192, 3), (64, 40, 64, 1)]:
        for exact in (True, False):
            a = to8(rng.choice(EXACT_VALS, m * k * batch), fa) if exact else finite_bytes(rng, m * k * batch, fa)
            bt = to8(rng.choice(EXACT_VALS, n * k), fb) if exact else finite_bytes(rng, n * k, fb)
            blob, dense = _pruned_pair_fp8(gpu, a, fa, m, k, batch)
            dB = dev8(bt, fb)
            rs = torch.from_numpy(rng.uniform(0.5, 2.0, m).astype(np.float32)).cuda()
            Cs = torch.empty(batch * m * n, dtype=odt(out), device="cuda")
            Cd = torch.full_like(Cs, 3.0)
            alpha = 1.0 if exact else 0.75
            gpu.spmma_fp8(blob, dB, Cs, m, n, k, batch, alpha=alpha, row_scale=None if exact else rs, a_dtype=tdt(fa))
            gpu.gemm_rowmajor_fp8(dense, dB, Cd, m, n, k, batch=batch, alpha=alpha, row_scale=None if exact else rs)
            torch.cuda.synchronize()
            if exact:
                assert same_bits(Cs, Cd), f"{fa} x {fb} -> {out} {(m, n, k, batch)}: dense != sparse on exact operands"
                continue
            prod, absprod = ref_fp8(bytes_of(dense).reshape(batch, m, k), fa, bt, fb, n, k, batch, True)
            s = alpha * rs.cpu().numpy().astype(np.float64)[None, :, None]
            ref, scale = s * prod, np.abs(s) * absprod
            bound = ROUND[out] * np.abs(ref) + (2.0 * ksteps(k) + 4.0) * 2.0 ** -24 * scale + TINY[out]
            for name, C in (("dense", Cd), ("sparse", Cs)):
                got = host(C).reshape(ref.shape)
                ratio = float((np.abs(got - ref) / bound).max())
                assert np.isfinite(got).all() and ratio <= 1.0, f"{fa} x {fb} -> {out} {(m, n, k, batch)} {name}: err/bound {ratio:.3f}"


@pytest.mark.parametrize("shape", [(196, 256, 512, 2), (130, 72, 192, 3), (64, 40, 64, 1)])
def test_gemm_i8_vs_spmma_i8_on_the_pruned_matrix(gpu, shape):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(sum(shape))
    a = torch.from_numpy(rng.integers(-128, 128, batch * m * k).astype(np.int8)).cuda()
    bt = torch.from_numpy(rng.integers(-128, 128, n * k).astype(np.int8)).cuda()
    blob = torch.empty(gpu.compress24_size(m, k, 1, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(a, m, k, k, batch, m * k, blob)  # int8 operands: sm_compress24_i8
    dense = torch.zeros_like(a)
    gpu.decompress24(blob, m, k, k, batch, m * k, dense)
    Cs = torch.empty(batch * m * n, dtype=torch.int32, device="cuda")
    Cd = torch.full_like(Cs, 7)
    gpu.spmma_i8(blob, bt, Cs, m, n, k, batch)
    gpu.gemm_rowmajor_i8(dense, bt, Cd, m, n, k, batch=batch)
    assert torch.equal(Cs, Cd)
    Qs = torch.empty(batch * m * n, dtype=torch.int8, device="cuda")
    Qd = torch.full_like(Qs, 5)
    gpu.spmma_i8_q(blob, bt, Qs, m, n, k, 1.0 / 3000.0, batch)
    gpu.gemm_rowmajor_i8_q(dense, bt, Qd, m, n, k, 1.0 / 3000.0, batch=batch)
    assert torch.equal(Qs, Qd)


# ---------------------------------------------------------------------------------------------
# epilogue, batches, shapes
# ---------------------------------------------------------------------------------------------
# (m, n, k, batch, lda, strideA, shared B): ragged m and n, n < 16, k = 64 (one plane), lda > k, a gap between the A
# matrices, the folded tall-matrix case (shared B, contiguous A and C)
# (the padding here is ordinary finite data and C is exactly sized; tests/test_gpu_strided8.py runs the same entry points with
# NaN padding, sentinel-guarded C, strideB / strideC gaps and offset bases)
CASES = [(64, 64, 128, 1, 128, None, True), (130, 72, 192, 3, 192, None, True), (130, 72, 192, 3, 192, None, False),
         (33, 9, 64, 2, 64, None, True), (7, 5, 320, 1, 336, None, True), (100, 130, 256, 2, 272, None, True),
         (100, 130, 256, 2, 272, 100 * 272 + 64, True), (61, 200, 128, 4, 160, 61 * 160 + 32, False), (1, 1, 64, 1, 64, None, True),
         (258, 64, 576, 2, 576, None, True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join("-" if v is None else str(v) for v in c))
@pytest.mark.parametrize("out", OUTS)
def test_gemm_fp8_epilogue_and_shapes(gpu, case, out):
    import torch
    m, n, k, batch, lda, strideA, shared = case
    strideA = m * lda if strideA is None else strideA
    rng = np.random.default_rng(m * 7 + n * 3 + k + batch + OUTS.index(out))
    a = finite_bytes(rng, (batch - 1) * strideA + m * lda, "e4m3")
    bt = finite_bytes(rng, n * k * (1 if shared else batch), "e5m2")
    A3 = a_rows(a, m, k, lda, batch, strideA)
    prod, absprod = ref_fp8(A3, "e4m3", bt, "e5m2", n, k, batch, shared)
    for alpha, beta, with_rs in ((1.0, 0.0, False), (0.75, 0.5, True), (-1.5, 1.0, True), (2.0, -0.25, False)):
        C0 = torch.from_numpy(rng.uniform(-4, 4, batch * m * n).astype(np.float32)).to(odt(out)).cuda()
        C = C0.clone()
        rs = torch.from_numpy(rng.uniform(0.25, 2.0, m).astype(np.float32)).cuda() if with_rs else None
        gpu.gemm_rowmajor_fp8(dev8(a, "e4m3"), dev8(bt, "e5m2"), C, m, n, k, lda=lda, batch=batch, strideA=strideA,
                              strideB=0 if shared else n * k, alpha=alpha, beta=beta, row_scale=rs)
        s = alpha * (rs.cpu().numpy().astype(np.float64)[None, :, None] if with_rs else 1.0)
        c0 = host(C0).reshape(prod.shape)
        ref = s * prod + beta * c0
        scale = np.abs(s) * absprod + abs(beta) * np.abs(c0)
        got = host(C).reshape(prod.shape)
        bound = ROUND[out] * np.abs(ref) + (2.0 * ksteps(k) + 4.0) * 2.0 ** -24 * scale + TINY[out]
        ratio = float((np.abs(got - ref) / bound).max())
        assert np.isfinite(got).all() and ratio <= 1.0, f"{case} -> {out} alpha={alpha} beta={beta} rs={with_rs}: err/bound {ratio:.3f}"


def test_gemm_fp8_beta_zero_does_not_read_c(gpu):
    """beta == 0: C's old contents (NaN here) never reach the result"""
    import torch
    m, n, k = 96, 80, 128
    rng = np.random.default_rng(2)
    a, bt = to8(rng.choice(EXACT_VALS, m * k), "e4m3"), to8(rng.choice(EXACT_VALS, n * k), "e4m3")
    for out in OUTS:
        C = torch.full((m * n,), float("nan"), dtype=odt(out), device="cuda")
        gpu.gemm_rowmajor_fp8(dev8(a, "e4m3"), dev8(bt, "e4m3"), C, m, n, k, alpha=0.5)
        prod, _ = ref_fp8(a.reshape(1, m, k), "e4m3", bt, "e4m3", n, k, 1, True)
        assert np.array_equal(host(C).reshape(prod.shape), rounded(0.5 * prod, out)), out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join("-" if v is None else str(v) for v in c))
def test_gemm_i8_shapes(gpu, case):
    import torch
    m, n, k, batch, lda, strideA, shared = case
    strideA = m * lda if strideA is None else strideA
    rng = np.random.default_rng(m + 5 * n + k + batch)
    a = rng.integers(-128, 128, (batch - 1) * strideA + m * lda).astype(np.int8)
    bt = rng.integers(-128, 128, n * k * (1 if shared else batch)).astype(np.int8)
    want = _i8_ref(a_rows(a, m, k, lda, batch, strideA), bt, n, k, batch, shared)
    C = torch.full((batch * m * n,), -1, dtype=torch.int32, device="cuda")
    dA, dB = torch.from_numpy(a).cuda(), torch.from_numpy(bt).cuda()
    gpu.gemm_rowmajor_i8(dA, dB, C, m, n, k, lda=lda, batch=batch, strideA=strideA, strideB=0 if shared else n * k)
    assert np.array_equal(C.cpu().numpy().astype(np.int64).reshape(want.shape), want)
    Q = torch.full((batch * m * n,), 1, dtype=torch.int8, device="cuda")
    gpu.gemm_rowmajor_i8_q(dA, dB, Q, m, n, k, 1.0 / 2048.0, lda=lda, batch=batch, strideA=strideA, strideB=0 if shared else n * k)
    wq = np.clip(np.rint(np.float32(1.0 / 2048.0) * want.astype(np.float32)), -128, 127).astype(np.int8)
    assert np.array_equal(Q.cpu().numpy().reshape(want.shape), wq)


# ---------------------------------------------------------------------------------------------
# specials
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,special", [("e4m3", 0x7F), ("e4m3", 0xFF), ("e5m2", 0x7E), ("e5m2", 0x7C), ("e5m2", 0xFC)])
@pytest.mark.parametrize("out", OUTS)
def test_gemm_fp8_specials_reach_their_row(gpu, fa, special, out):
    """a NaN or an e5m2 inf in row r of A makes row r of C non-finite (inf x 0 = NaN: B holds zeros) and leaves every other
    row exact; -0 (0x80) behaves as +0"""
    import torch
    m, n, k, batch = 70, 48, 192, 2
    rng = np.random.default_rng(special + OUTS.index(out))
    a = to8(rng.choice(EXACT_VALS, m * k * batch), fa)
    bt = to8(rng.choice(EXACT_VALS, n * k), "e4m3")
    bad_rows = [3, m + 41]
    for r, c in zip(bad_rows, (5, 130)):
        a[r * k + c] = special
    C = torch.empty(batch * m * n, dtype=odt(out), device="cuda")
    gpu.gemm_rowmajor_fp8(dev8(a, fa), dev8(bt, "e4m3"), C, m, n, k, batch=batch)
    got = host(C).reshape(batch * m, n)
    clean = a.copy()
    for r, c in zip(bad_rows, (5, 130)):
        clean[r * k + c] = 0
    prod, _ = ref_fp8(clean.reshape(batch, m, k), fa, bt, "e4m3", n, k, batch, True)
    want = rounded(prod.reshape(batch * m, n), out)
    good = np.setdiff1d(np.arange(batch * m), bad_rows)
    assert np.array_equal(got[good], want[good])
    for r in bad_rows:
        assert not np.isfinite(got[r]).any(), f"row {r}"
        if (special & 0x7F) != 0x7C:  # NaN: NaN everywhere in the row
            assert np.isnan(got[r]).all(), f"row {r}"
    # -0 for every zero of A: the same values as +0
    negz = a.copy()
    negz[(negz == 0) & (rng.random(negz.size) < 0.7)] = 0x80
    negz[[r * k + c for r, c in zip(bad_rows, (5, 130))]] = 0x80
    C2 = torch.empty_like(C)
    gpu.gemm_rowmajor_fp8(dev8(negz, fa), dev8(bt, "e4m3"), C2, m, n, k, batch=batch)
    assert np.array_equal(host(C2).reshape(batch * m, n), want)


# ---------------------------------------------------------------------------------------------
# graph capture, full size, driver
# ---------------------------------------------------------------------------------------------
def test_gemm_b8_graph_capture_replays(gpu):
    import torch
    m, n, k, batch = 196, 256, 512, 4
    g = torch.Generator(device="cuda").manual_seed(9)
    A = (torch.rand(batch * m * k, generator=g, device="cuda") * 2 - 1).to(torch.float8_e5m2)
    Bt = (torch.rand(n * k, generator=g, device="cuda") * 2 - 1).to(torch.float8_e4m3fn)
    rs = torch.rand(m, generator=g, device="cuda") + 0.5
    C = torch.empty(batch * m * n, dtype=torch.bfloat16, device="cuda")
    Ai = torch.randint(-128, 128, (batch * m * k,), generator=g, device="cuda", dtype=torch.int8)
    Bi = torch.randint(-128, 128, (n * k,), generator=g, device="cuda", dtype=torch.int8)
    Ci = torch.empty(batch * m * n, dtype=torch.int32, device="cuda")
    Cq = torch.empty(batch * m * n, dtype=torch.int8, device="cuda")

    def step():
        gpu.gemm_rowmajor_fp8(A, Bt, C, m, n, k, batch=batch, row_scale=rs, alpha=0.5)
        gpu.gemm_rowmajor_i8(Ai, Bi, Ci, m, n, k, batch=batch)
        gpu.gemm_rowmajor_i8_q(Ai, Bi, Cq, m, n, k, 1.0 / 1024.0, batch=batch)
    step()
    torch.cuda.synchronize()
    want = (C.clone(), Ci.clone(), Cq.clone())
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    C.fill_(7.0)
    Ci.fill_(7)
    Cq.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(C.view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(Ci, want[1]) and torch.equal(Cq, want[2])


def _resnet50_non_stem():
    import csv
    with open(os.path.join(ROOT, "datasets", "resnet50.csv"), newline="") as fh:
        rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(fh))[1:] if r]
    return sorted(s for s in set(rows) if s[2] % 64 == 0)


@pytest.mark.parametrize("shape", _resnet50_non_stem(), ids=lambda s_: "x".join(map(str, s_)))
def test_gemm_fp8_full_size_resnet50(gpu, shape):
    """b = 32, shared B, bf16 out: every element against the fp32 product of the decoded operands (on the GPU), within the
    bf16 rounding plus two fp32 accumulations' bound"""
    import torch
    m, n, k, batch = shape
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    A = (torch.rand(batch * m * k, generator=g, device="cuda") * 4 - 2).to(torch.float8_e4m3fn)
    Bt = (torch.rand(n * k, generator=g, device="cuda") * 4 - 2).to(torch.float8_e4m3fn)
    C = torch.empty(batch * m * n, dtype=torch.bfloat16, device="cuda")
    gpu.gemm_rowmajor_fp8(A, Bt, C, m, n, k, batch=batch)
    Af, Bf = A.float().view(batch * m, k), Bt.float().view(n, k)
    ref = Af @ Bf.t()
    absref = Af.abs() @ Bf.abs().t()
    del Af
    bound = ROUND["bf16"] * ref.abs() + 4.0 * ksteps(k) * 2.0 ** -24 * absref + TINY["bf16"]
    err = (C.view(batch * m, n).float() - ref).abs()
    ratio = float((err / bound).max())
    assert torch.isfinite(C.float()).all() and ratio <= 1.0, f"{shape}: err/bound {ratio:.3f}"


def test_gemm_fp8_driver_cli_contract(gpu):
    bins = os.path.join(ROOT, "examples", "bin")
    if not os.path.exists(os.path.join(bins, "gemm_fp8")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "-j4"], check=True, capture_output=True)

    def run(*args):
        return subprocess.run([os.path.join(bins, "gemm_fp8")] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    for argv in [(196, 64, 128, 4), (784, 256, 1152, 2), (131, 72, 192, 3)]:
        out = run(*argv)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.strip().splitlines()
        assert lines[0].split(":")[0] == "GEMM Time (ms)" and float(lines[0].split(":")[1]) > 0.0
        assert "Correct: yes" in out.stdout
    bad = run(1, 2)
    assert bad.returncode != 0 and "Usage: ./gemm_fp8 m n k b" in bad.stdout
