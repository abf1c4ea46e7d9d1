"""GPU parity tests (-m gpu): every HIP entry point, called through the C ABI, against the CPU oracle
on the same seeded inputs.  Bit-exact for masks / pruned matrices / compressed blobs (integer and
byte work); GEMM outputs within north_star's tolerance (1e-2 relative for fp16, 1e-3 for fp32, relative to
sum_k |a*b|, the natural scale of the accumulation) AND within the bound the arithmetic itself
allows (check_close: one rounding of the output type + k fp32 accumulation steps), which is ~50x tighter."""
import numpy as np
import pytest

from parity_testlib import (ACC, FP16_TOL, FP32_TOL, MARGINS, ROUND, SPLIT_TOL, TINY, _sk_ran, _sk_ws, bf16_bits, bf16_f64, bits, check_close, host, rand,
                            split_bound, to_dev, torch_dtype, write_margin_report)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# (a1) positional sparsify
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
@pytest.mark.parametrize("shape", [(4, 4), (3, 5), (2, 2), (1, 7), (0, 4), (196, 512), (784, 147), (513, 1031), (64, 6)])
@pytest.mark.parametrize("sf", [0.0, 0.25, 0.5, 0.75, 1.0])
def test_sparsify_positional(gpu, orc, dtype, shape, sf):
    import torch
    m, n = shape
    rng = np.random.default_rng(m * 1000 + n)
    w = rand(rng, m * n, dtype) + dtype(2)  # no zeros in the input, so zeroed positions are visible
    mask = np.full(m * n, 99, dtype=np.uint64)
    ew, em = w.copy(), mask.copy()
    orc.sparsify_positional(ew, em, m, n, sf)
    dw = to_dev(w) if m * n else torch.empty(0, dtype=torch_dtype(dtype), device="cuda")
    dm = torch.full((m * n,), 99, dtype=torch.int64, device="cuda")
    if m * n:
        gpu.sparsify(dw, dm, m, n, sf)
        assert np.array_equal(bits(host(dw)), bits(ew))
        assert np.array_equal(host(dm).view(np.uint64), em)


def test_sparsify_positional_generic_block_and_unaligned(gpu, orc):
    import torch
    m, n = 8, 12
    w = np.arange(1, m * n + 1, dtype=np.float32)
    for (bm, bn, sf) in [(1, 4, 0.25), (2, 2, 0.5)]:
        ew, em = w.copy(), np.zeros(m * n, dtype=np.uint64)
        orc.sparsify_positional(ew, em, m, n, sf, bm, bn)
        # an element-offset view: base pointer only 4-byte aligned -> generic path
        buf = torch.zeros(m * n + 1, dtype=torch.float32, device="cuda")
        dw = buf[1:]
        dw.copy_(torch.from_numpy(w))
        dm = torch.zeros(m * n, dtype=torch.int64, device="cuda")
        gpu.sparsify(dw, dm, m, n, sf, bm, bn)
        assert np.array_equal(host(dw), ew) and np.array_equal(host(dm).view(np.uint64), em)
    with pytest.raises(gpu.SparsifymeError):
        gpu.sparsify(dw, dm, m, n, 1.0, 1, 4)  # would index outside the buffer


# ---------------------------------------------------------------------------------------------
# (a2) prune STRIP / TILE + check
# ---------------------------------------------------------------------------------------------
PRUNE_SHAPES = [(1, 4, 4), (4, 4, 4), (3, 5, 5), (7, 147, 147), (10, 147, 152), (16, 64, 64), (33, 72, 80),
                (196, 512, 512), (784, 1024, 1024), (130, 260, 264), (5, 3, 3), (257, 8, 8),
                # round 6: the span form of TILE (16-bit types, ld == k, ragged rows): several spans, a short last span that ends off a
                # 16-byte boundary, m % 4 != 0, k % 4 != 0, and two wide rows -- 1022 and 1026 BOTH run the span form (it takes every k <= 4096
                # and picks 8 to 64 rows per span; the element-wise kernel on contiguous ragged rows is tests/test_gpu_prune_classes.py's, k = 4097)
                (129, 147, 147), (100, 30, 30), (64, 1022, 1022), (40, 1026, 1026), (3136, 147, 147)]
# the kernel class (sm_prune24_form) of the rows above whose comment names one: TILE on fp16 (fp32 has no span form: element-wise, ld odd)
PRUNE_SHAPE_FORMS = {(129, 147, 147): "span", (100, 30, 30): "span", (64, 1022, 1022): "span", (40, 1026, 1026): "span", (3136, 147, 147): "span"}


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("alg", [0, 1], ids=["tile", "strip"])
@pytest.mark.parametrize("shape", PRUNE_SHAPES)
@pytest.mark.parametrize("kind", ["uniform", "ties"])
def test_prune24(gpu, orc, dtype, alg, shape, kind):
    import torch
    m, k, ld = shape
    rng = np.random.default_rng(m * 7919 + k * 13 + alg)
    A = rand(rng, m * ld, dtype, kind)
    want = orc.prune24(bits(A), m, k, ld, alg)
    dA = to_dev(A)
    dOut = torch.zeros_like(dA)
    dOut.copy_(dA)  # padding columns must stay as they are
    if shape in PRUNE_SHAPE_FORMS and alg == 0:
        want_form = PRUNE_SHAPE_FORMS[shape] if dtype == np.float16 else ("element_vec" if ld % 4 == 0 else "element_scalar")
        assert gpu.prune24_form(dA, dOut, m, k, ld, A.itemsize, alg) == want_form, f"{shape} reaches another kernel"
    gpu.prune24(dA, dOut, m, k, ld, alg)
    assert np.array_equal(bits(host(dOut)), want), "out-of-place prune differs from the oracle"
    gpu.prune24(dA, dA, m, k, ld, alg)  # in place, as spmma.hxx:86 does
    assert np.array_equal(bits(host(dA)), want), "in-place prune differs from the oracle"
    valid = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    gpu.prune24_check(dA, m, k, ld, valid)
    assert int(host(valid)[0]) == 0 == orc.prune24_check(want, m, k, ld)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_prune_check_flags_dense_and_single_bad_strip(gpu, orc, dtype):
    import torch
    m, k = 300, 512
    rng = np.random.default_rng(1)
    A = rand(rng, m * k, dtype, "u01") + dtype(0.5)
    valid = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu.prune24_check(to_dev(A), m, k, k, valid)
    assert int(host(valid)[0]) == 1 == orc.prune24_check(bits(A), m, k, k)
    P = orc.prune24(bits(A), m, k, k, 1).view(dtype).copy()
    P[(m - 1) * k + k - 4:(m - 1) * k + k] = 1  # one bad strip at the very end
    gpu.prune24_check(to_dev(P), m, k, k, valid)
    assert int(host(valid)[0]) == 1 == orc.prune24_check(bits(P), m, k, k)


def test_prune_special_values(gpu, orc):
    a = np.array([1.0, np.nan, np.inf, 2.0, -0.0, 0.0, -0.0, 0.0, np.nan, np.nan, np.nan, 1.0,
                  6e-8, -6e-8, 6e-8, 0.0], dtype=np.float16)
    for alg in (0, 1):
        A = np.tile(a, 4)  # 4 x 16
        want = orc.prune24(bits(A), 4, 16, 16, alg)
        dA = to_dev(A)
        gpu.prune24(dA, dA, 4, 16, 16, alg)
        assert np.array_equal(bits(host(dA)), want)


# ---------------------------------------------------------------------------------------------
# (a3) compress / decompress
# ---------------------------------------------------------------------------------------------
COMPRESS_SHAPES = [(1, 4, 4, 1), (5, 147, 147, 3), (5, 147, 152, 2), (16, 64, 64, 2), (196, 512, 512, 2),
                   (33, 72, 80, 1), (130, 1152, 1152, 1), (7, 8, 8, 5), (3, 200, 200, 1)]


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", COMPRESS_SHAPES)
@pytest.mark.parametrize("pruned_first", [False, True])
def test_compress24_bit_exact(gpu, orc, dtype, shape, pruned_first):
    import torch
    m, k, ld, batch = shape
    rng = np.random.default_rng(m + 31 * k + batch)
    stride = m * ld + (8 if ld % 8 == 0 else 0)  # a padded batch stride
    A = rand(rng, batch * stride, dtype, "ties" if m % 2 else "uniform")
    if pruned_first:
        for b in range(batch):
            seg = A[b * stride:b * stride + m * ld]
            seg[:] = orc.prune24(bits(seg), m, k, ld, 0).view(dtype)  # TILE-pruned input, as spmma feeds it
    want = orc.compress24(bits(A), m, k, ld, batch, stride)
    blob = torch.full((gpu.compress24_size(m, k, A.dtype.itemsize, batch),), 0xAB, dtype=torch.uint8, device="cuda")
    assert blob.numel() == want.size
    gpu.compress24(to_dev(A), m, k, ld, batch, stride, blob)
    assert np.array_equal(host(blob), want), "compressed blob differs from the oracle"
    # decompress on the GPU == oracle decompress == STRIP-pruned input
    D = torch.zeros(batch * stride, dtype=torch_dtype(dtype), device="cuda")
    gpu.decompress24(blob, m, k, ld, batch, stride, D)
    wantD = orc.decompress24(want, m, k, ld, bits(A).dtype, batch, stride)
    assert np.array_equal(bits(host(D)), wantD)


# ---------------------------------------------------------------------------------------------
# (a2 + a3) prune -> check -> compress in one pass, as sparsifyme::spmma() runs them (spmma.hxx:82-104)
# ---------------------------------------------------------------------------------------------
PC_SHAPES = [(4, 64, 64, 1, 0), (196, 512, 512, 2, 0), (130, 128, 128, 3, 0), (130, 128, 136, 3, 24), (7, 64, 64, 5, 0),
             (784, 1152, 1152, 1, 0), (33, 576, 576, 2, 0), (257, 64, 72, 1, 0),
             # shapes the one-pass kernel does not take (k % 64 != 0, odd leading dimension): the three-launch sequence
             (12, 147, 147, 2, 0), (20, 72, 72, 2, 0), (9, 8, 8, 3, 0),
             # round 6: ragged rows through the span form of TILE -- one tall matrix (flag raised in the same pass) and m % 4 != 0 (per batch matrix)
             (196, 147, 147, 3, 0), (130, 147, 147, 2, 0)]


@pytest.mark.parametrize("alg", [0, 1], ids=["tile", "strip"])
@pytest.mark.parametrize("shape", PC_SHAPES)
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_prune_compress_one_pass_bit_exact(gpu, orc, alg, shape, bf):
    """sm_prune24_compress24_*: pruned A, blob and flag must be the bytes of prune (per batch matrix) + check +
    compress of the oracle; in place and out of place; A_out / blob / flag individually optional."""
    import torch
    m, k, ld, batch, pad = shape
    stride = m * ld + pad
    rng = np.random.default_rng(m * 31 + k * 7 + alg + batch)
    if bf:
        A = bf16_bits(rng, batch * stride, "ties" if m % 2 else "uniform")
    else:
        A = bits(rand(rng, batch * stride, np.float16, "ties" if m % 2 else "uniform"))
    if m == 196:   # specials: NaN, inf, signed zeros, subnormals
        A[:16] = np.array([1.0, np.nan, np.inf, 2.0, -0.0, 0.0, -0.0, 0.0, np.nan, np.nan, np.nan, 1.0, 6e-8, -6e-8, 6e-8, 0.0],
                          dtype=np.float16).view(np.uint16) if not bf else np.array([0x3f80, 0x7fc0, 0x7f80, 0x4000, 0x8000, 0, 0x8000, 0,
                                                                                      0x7fc1, 0xffc0, 0x7fff, 0x3f80, 1, 0x8001, 1, 0], dtype=np.uint16)
    want = A.copy()
    for b in range(batch):
        seg = want[b * stride:b * stride + m * ld]
        seg[:] = orc.prune24(seg.copy(), m, k, ld, alg, bf16=bf)
    want_blob = orc.compress24(want, m, k, ld, batch, stride)
    todev = (lambda x: bf16_dev(x)) if bf else (lambda x: torch.from_numpy(x.view(np.int16)).cuda().view(torch.float16))
    tohost = (lambda t: bf16_host(t)) if bf else (lambda t: bits(host(t)))
    nbytes = gpu.compress24_size(m, k, 2, batch)
    for in_place in (False, True):
        dA = todev(A)
        dOut = dA if in_place else todev(A)
        blob = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        valid = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        gpu.prune24_compress24(dA, dOut, m, k, ld, batch, stride, blob, valid, alg)
        assert np.array_equal(tohost(dOut), want), f"pruned A differs (in_place={in_place})"
        if not in_place:
            assert np.array_equal(tohost(dA), A), "out-of-place call touched its input"
        assert np.array_equal(host(blob), want_blob), "blob differs from compress(prune(A))"
        assert int(host(valid)[0]) == 0
        # the one-pass kernel's own flag is by construction on its fast path: the INDEPENDENT inspection
        # of what was written is sm_prune24_check_* on the output, per batch matrix
        for b in range(batch):
            v2 = torch.full((1,), 9, dtype=torch.int32, device="cuda")
            gpu.prune24_check(dOut[b * stride:], m, k, ld, v2)
            assert int(host(v2)[0]) == 0
    # optional outputs
    blob2 = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device="cuda")
    dA = todev(A)
    if alg == 1 or (k % 64 == 0 and ld % 8 == 0 and stride % 8 == 0):   # TILE without A_out needs the one-pass kernel
        gpu.prune24_compress24(dA, None, m, k, ld, batch, stride, blob2, None, alg)
        assert np.array_equal(host(blob2), want_blob) and np.array_equal(tohost(dA), A)
    dOut = todev(A)
    gpu.prune24_compress24(dA, dOut, m, k, ld, batch, stride, None, None, alg)
    assert np.array_equal(tohost(dOut), want)


@pytest.mark.parametrize("alg", [0, 1], ids=["tile", "strip"])
@pytest.mark.parametrize("shape", PC_SHAPES)
def test_prune_compress_one_pass_f32_bit_exact(gpu, orc, alg, shape):
    """sm_prune24_compress24_f32 (round 3; the type the reference's driver instantiates, examples/spmma.cu:24): pruned A,
    blob and flag are the bytes of the oracle's prune (per batch matrix) + check + compress; in place and out of place;
    outputs individually optional; ties, NaN / inf / signed zeros / subnormals."""
    import torch
    m, k, ld, batch, pad = shape
    stride = m * ld + pad
    rng = np.random.default_rng(m * 29 + k * 11 + alg + batch)
    A = rand(rng, batch * stride, np.float32, "ties" if m % 2 else "uniform")
    if m == 196:
        A[:16] = np.array([1.0, np.nan, np.inf, 2.0, -0.0, 0.0, -0.0, 0.0, np.nan, np.nan, np.nan, 1.0, 1e-45, -1e-45, 1e-45, 0.0], dtype=np.float32)
    Ab = A.view(np.uint32).copy()
    want = Ab.copy()
    for b in range(batch):
        seg = want[b * stride:b * stride + m * ld]
        seg[:] = orc.prune24(seg.copy(), m, k, ld, alg)
    want_blob = orc.compress24(want, m, k, ld, batch, stride)
    todev = lambda x: torch.from_numpy(x.view(np.int32)).cuda().view(torch.float32)
    tohost = lambda t: host(t.view(torch.int32)).view(np.uint32)
    nbytes = gpu.compress24_size(m, k, 4, batch)
    for in_place in (False, True):
        dA = todev(Ab)
        dOut = dA if in_place else todev(Ab)
        blob = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        valid = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        gpu.prune24_compress24(dA, dOut, m, k, ld, batch, stride, blob, valid, alg)
        assert np.array_equal(tohost(dOut), want), f"pruned A differs (in_place={in_place})"
        if not in_place:
            assert np.array_equal(tohost(dA), Ab), "out-of-place call touched its input"
        assert np.array_equal(host(blob), want_blob), "blob differs from compress(prune(A))"
        assert int(host(valid)[0]) == 0
    blob2 = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device="cuda")
    dA = todev(Ab)
    if alg == 1 or (k % 64 == 0 and ld % 4 == 0 and stride % 4 == 0):
        gpu.prune24_compress24(dA, None, m, k, ld, batch, stride, blob2, None, alg)
        assert np.array_equal(host(blob2), want_blob) and np.array_equal(tohost(dA), Ab)
    dOut = todev(Ab)
    gpu.prune24_compress24(dA, dOut, m, k, ld, batch, stride, None, None, alg)
    assert np.array_equal(tohost(dOut), want)


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_tile_prune_on_gpu_equals_the_exhaustive_statement_on_ordinary_data(gpu, orc, bf):
    """The TILE rule is frozen in its two-level statement (oracle tile_select; INTEGRATION.md "TILE rule version 2"); where
    the pair sums are exact -- 16-bit data of ordinary dynamic range -- it must pick the lexicographically first maximal
    pattern of the round-1 exhaustive statement, which the oracle keeps as tile_select_exhaustive.  Here the GPU kernels
    (prune and the one-pass prune+compress) are held against that exhaustive statement tile by tile."""
    import torch
    m, k = 64, 128
    rng = np.random.default_rng(77 + bf)
    if bf:
        A = bf16_bits(rng, m * k, "uniform")
        mag = torch.from_numpy(A.view(np.int16)).view(torch.bfloat16).float().abs().numpy().reshape(m, k)
        dA = bf16_dev(A)
    else:
        Af = rand(rng, m * k, np.float16)
        A = bits(Af)
        mag = np.abs(Af.astype(np.float32)).reshape(m, k)
        dA = to_dev(Af)
    out = torch.empty_like(dA)
    gpu.prune24(dA, out, m, k, k, gpu.PRUNE_TILE)
    out2 = torch.empty_like(dA)
    gpu.prune24_compress24(dA, out2, m, k, k, 1, m * k, None, None, gpu.PRUNE_TILE)
    got = (bf16_host(out) if bf else bits(host(out))).reshape(m, k)
    got2 = (bf16_host(out2) if bf else bits(host(out2))).reshape(m, k)
    Ab = A.reshape(m, k)
    for r0 in range(0, m, 4):
        for c0 in range(0, k, 4):
            two, exh, s2, se = orc.tile_select_both(mag[r0:r0 + 4, c0:c0 + 4])
            assert two == exh and s2 == se   # ordinary range: the two statements coincide
            want = Ab[r0:r0 + 4, c0:c0 + 4].copy()
            for r in range(4):
                for c in range(4):
                    if not (exh >> (4 * r + c)) & 1:
                        want[r, c] = 0
            assert np.array_equal(got[r0:r0 + 4, c0:c0 + 4], want) and np.array_equal(got2[r0:r0 + 4, c0:c0 + 4], want)


def test_prune_compress_full_size_resnet50_layer(gpu, orc):
    """One ResNet-50 layer at b = 32 (784 x 2304): the one-pass TILE kernel equals the three separate launches bit for
    bit, and sampled tile rows equal the oracle."""
    import torch
    m, k, batch = 784, 2304, 32
    dA = torch.empty(batch * m * k, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dA, 0xA91, -1.0, 1.0)
    P1 = dA.clone()
    gpu.prune24(P1, P1, batch * m, k, k, gpu.PRUNE_TILE)
    blob1 = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(P1, m, k, k, batch, m * k, blob1)
    P2 = torch.empty_like(dA)
    blob2 = torch.empty_like(blob1)
    valid = torch.ones(1, dtype=torch.int32, device="cuda")
    gpu.prune24_compress24(dA, P2, m, k, k, batch, m * k, blob2, valid, gpu.PRUNE_TILE)
    assert torch.equal(P1.view(torch.int16), P2.view(torch.int16)) and torch.equal(blob1, blob2) and int(valid.item()) == 0
    rows = 16
    for b in (0, batch - 1):
        seg = bits(host(dA[b * m * k: b * m * k + rows * k]))
        want = orc.prune24(seg, rows, k, k, orc.TILE)
        assert np.array_equal(bits(host(P2[b * m * k: b * m * k + rows * k])), want)


# ---------------------------------------------------------------------------------------------
# (a4) spmma and (a5) dense gemm
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _parity_margin_report():
    yield
    if not MARGINS:
        return
    worst = sorted(MARGINS, key=lambda t: -t[1])[:25]
    lines = [f"{len(MARGINS)} GEMM-type comparisons against the fp64 oracle; err / (ROUND*|ref| + 2k*ACC*sum|ab|), worst first:"]
    lines += [f"  {r:6.3f}  {w}" for w, r in worst]
    write_margin_report(lines)


def test_mfma_lane_maps_with_identity_and_asymmetric_b(gpu, orc):
    """A = I (pruned 2:4-compatible: one non-zero per strip) with an ASYMMETRIC integer B: a swapped
    row/col, a wrong k-slot or a wrong index nibble anywhere shows up exactly."""
    import torch
    for (m, n, k) in [(128, 64, 128), (128, 128, 256), (200, 72, 192), (64, 192, 64)]:
        A = np.zeros((m, k), dtype=np.float16)
        for i in range(m):
            A[i, (i * 5 + 3) % k] = 1.0          # one element per row, varying strip position
            A[i, (i * 11 + 64) % k] += 2.0
        B = ((np.arange(k)[:, None] * 3 + np.arange(n)[None, :] * 7) % 61 - 30).astype(np.float16)
        want = A.astype(np.float64) @ B.astype(np.float64)
        assert orc.prune24_check(bits(A.reshape(-1)), m, k, k) == 0
        blob = torch.empty(gpu.compress24_size(m, k, 2), dtype=torch.uint8, device="cuda")
        dA, dB = to_dev(A.reshape(-1)), to_dev(B.reshape(-1))
        gpu.compress24(dA, m, k, k, 1, m * k, blob)
        C = torch.zeros(m * n, dtype=torch.float16, device="cuda")
        gpu.spmma(blob, dB, C, m, n, k)
        assert np.array_equal(host(C).astype(np.float64).reshape(m, n), want), f"spmma lane map {m}x{n}x{k}"
        C2 = torch.zeros(m * n, dtype=torch.float16, device="cuda")
        gpu.gemm_rowmajor(dA, dB, C2, m, n, k)
        assert np.array_equal(host(C2).astype(np.float64).reshape(m, n), want), f"dense lane map {m}x{n}x{k}"


SPMMA_SHAPES = [(128, 64, 128, 1), (196, 512, 256, 2), (130, 72, 200, 1), (784, 256, 1024, 1), (96, 64, 64, 3),
                (12544, 64, 147, 1), (3136, 128, 576, 1), (17, 8, 4, 1), (300, 136, 320, 2),
                # producer/consumer kernels (k >= 512) with row, column and batch tails; 256-row tiles (>= 16384 rows)
                (200, 136, 576, 3), (130, 64, 1152, 2), (16400, 136, 1024, 1), (8200, 256, 1088, 2), (2, 8, 512, 1)]


@pytest.mark.parametrize("shape", SPMMA_SHAPES)
@pytest.mark.parametrize("shared_b", [True, False])
def test_spmma_f16_vs_oracle(gpu, orc, shape, shared_b):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + n + k)
    A = rand(rng, batch * m * k, np.float16)
    nb = 1 if shared_b else batch
    B = rand(rng, nb * k * n, np.float16)
    strideB = 0 if shared_b else k * n
    dA = to_dev(A)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)   # fused prune + compress
    C = torch.zeros(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, to_dev(B), C, m, n, k, batch, strideB)
    ob = orc.compress24(bits(A), m, k, k, batch)
    assert np.array_equal(host(blob), ob)
    Cref = np.zeros(batch * m * n, dtype=np.uint16)
    orc.spmma(ob, bits(B), Cref, m, n, k, batch, strideB)
    # scale = sum_k |a*b| of the pruned A
    P = np.abs(orc.decompress24(ob, m, k, k, np.uint16, batch).view(np.float16).astype(np.float64)).reshape(batch, m, k)
    Bm = np.abs(B.astype(np.float64)).reshape(nb, k, n)
    scale = np.stack([P[b] @ Bm[b if not shared_b else 0] for b in range(batch)]).reshape(-1)
    check_close(host(C), Cref.view(np.float16), scale, FP16_TOL, f"spmma {shape}", k)


@pytest.mark.parametrize("shape", [(256, 64, 147), (130, 136, 71), (512, 256, 1099)])
def test_spmma_k_tail_meets_zeros_not_a_clamped_row(gpu, orc, shape):
    """k % 64 != 0 on the fast (LDS-DMA) kernels: the blob's zero padding must be multiplied with zeros.  B's last
    valid row is +inf and never selected by A (column k-1 of A is zero, its strip holds larger values), so C is
    finite -- unless a kernel fed the padded stage from a clamped real row (0 * inf = NaN)."""
    import torch
    m, n, k = shape
    rng = np.random.default_rng(k)
    A = rand(rng, m * k, np.float16).reshape(m, k)
    A[:, k - 1] = 0
    s0 = (k - 1) // 4 * 4
    A[:, s0:k - 1] = np.where(np.abs(A[:, s0:k - 1]) < 0.25, np.float16(0.5), A[:, s0:k - 1])
    if k - 1 - s0 < 2:   # fewer than two other columns in the last strip: the zero would be kept (as a stored 0)
        pytest.skip("last strip too short for this construction")
    B = rand(rng, k * n, np.float16).reshape(k, n)
    B[k - 1, :] = np.inf
    blob = torch.empty(gpu.compress24_size(m, k, 2), dtype=torch.uint8, device="cuda")
    gpu.compress24(to_dev(A.reshape(-1)), m, k, k, 1, m * k, blob)
    C = torch.zeros(m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, to_dev(B.reshape(-1)), C, m, n, k)
    got = host(C)
    assert np.isfinite(got.astype(np.float32)).all(), "K tail multiplied the zero padding with a non-zero-page row"
    ob = orc.compress24(bits(A.reshape(-1)), m, k, k)
    Cref = np.zeros(m * n, dtype=np.uint16)
    orc.spmma(ob, bits(B.reshape(-1)), Cref, m, n, k)
    Bf = B.copy()
    Bf[k - 1, :] = 0
    scale = (np.abs(A.astype(np.float64)) @ np.abs(Bf.astype(np.float64))).reshape(-1)
    check_close(got, Cref.view(np.float16), scale, FP16_TOL, f"spmma k tail {shape}", k)


def test_spmma_alpha_beta(gpu, orc):
    import torch
    m, n, k = 140, 80, 192
    rng = np.random.default_rng(5)
    A, B = rand(rng, m * k, np.float16), rand(rng, k * n, np.float16)
    C0 = rand(rng, m * n, np.float16)
    blob = torch.empty(gpu.compress24_size(m, k, 2), dtype=torch.uint8, device="cuda")
    gpu.compress24(to_dev(A), m, k, k, 1, m * k, blob)
    C = to_dev(C0.copy())
    gpu.spmma(blob, to_dev(B), C, m, n, k, alpha=0.5, beta=-2.0)
    ob = orc.compress24(bits(A), m, k, k)
    Cref = bits(C0.copy())
    orc.spmma(ob, bits(B), Cref, m, n, k, alpha=0.5, beta=-2.0)
    scale = np.abs(A.astype(np.float64)).reshape(m, k) @ np.abs(B.astype(np.float64)).reshape(k, n) + 2 * np.abs(C0.astype(np.float64)).reshape(m, n)
    check_close(host(C), Cref.view(np.float16), scale.reshape(-1), FP16_TOL, "spmma alpha/beta", k)


GEMM_SHAPES = [(128, 64, 64, 1), (196, 512, 256, 2), (130, 72, 200, 1), (784, 256, 1024, 1), (64, 12544, 147, 1),
               (17, 9, 5, 2), (300, 136, 320, 2), (256, 64, 576, 3)]


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_rowmajor_f16_vs_oracle(gpu, orc, shape):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m * 3 + n * 5 + k)
    A, B = rand(rng, batch * m * k, np.float16), rand(rng, k * n, np.float16)
    C = torch.zeros(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.gemm_rowmajor(to_dev(A), to_dev(B), C, m, n, k, batch=batch)
    Cref = np.zeros(batch * m * n, dtype=np.uint16)
    orc.gemm_rowmajor(bits(A), bits(B), Cref, m, n, k, batch=batch)
    scale = (np.abs(A.astype(np.float64)).reshape(batch * m, k) @ np.abs(B.astype(np.float64)).reshape(k, n)).reshape(-1)
    check_close(host(C), Cref.view(np.float16), scale, FP16_TOL, f"gemm_rowmajor {shape}", k)


@pytest.mark.parametrize("shape", [(128, 64, 64, 2), (196, 512, 256, 2), (130, 72, 200, 3), (3136, 128, 576, 2), (12544, 64, 147, 1),
                                   # m % 8 == 4 on the LDS-DMA kernel (half-valid last chunk served from columns m-8 .. m-1)
                                   (44, 72, 128, 3), (196, 64, 64, 1), (1100, 136, 192, 2)])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
def test_gemm_batched_column_major_f16_vs_oracle(gpu, orc, shape, ab):
    """The reference's call: column-major, lda=m ldb=k ldc=m, device arrays of pointers, one shared B
    repeated `batch` times (examples/gemm.cu:40,60,86)."""
    import torch
    m, n, k, batch = shape
    alpha, beta = ab
    rng = np.random.default_rng(m + 2 * n + 3 * k)
    As = [rand(rng, m * k, np.float16) for _ in range(batch)]
    Bsh = rand(rng, k * n, np.float16)
    C0 = [rand(rng, m * n, np.float16) for _ in range(batch)]
    dAs = [to_dev(a) for a in As]
    dB = to_dev(Bsh)
    dCs = [to_dev(c.copy()) for c in C0]
    ptr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
    gpu.gemm_batched(ptr(dAs), ptr([dB] * batch), ptr(dCs), m, n, k, batch, "f16", alpha, beta)
    Cs = [bits(c.copy()) for c in C0]
    orc.gemm_batched([bits(a) for a in As], [bits(Bsh)] * batch, Cs, m, n, k, alpha, beta)
    Bm = np.abs(Bsh.astype(np.float64)).reshape(n, k).T            # column-major k x n
    for b in range(batch):
        Am = np.abs(As[b].astype(np.float64)).reshape(k, m).T      # column-major m x k
        scale = abs(alpha) * (Am @ Bm).T.reshape(-1) + abs(beta) * np.abs(C0[b].astype(np.float64))  # column-major m x n
        check_close(host(dCs[b]), Cs[b].view(np.float16), scale, FP16_TOL, f"gemm_batched {shape} batch {b}", k)


def test_spmma_equals_dense_gemm_of_pruned_on_gpu(gpu, orc):
    """spmma(compress(A), B) and gemm(prune(A), B) accumulate the same products in fp32: the results
    agree to a couple of fp16 ulps (they may differ in summation order only)."""
    import torch
    m, n, k, batch = 784, 256, 1152, 2
    rng = np.random.default_rng(9)
    A, B = rand(rng, batch * m * k, np.float16, "u01"), rand(rng, k * n, np.float16, "u01")
    dA, dB = to_dev(A), to_dev(B)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    C1 = torch.zeros(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, C1, m, n, k, batch)
    gpu.prune24(dA, dA, batch * m, k, k, gpu.PRUNE_STRIP)
    C2 = torch.zeros_like(C1)
    gpu.gemm_rowmajor(dA, dB, C2, m, n, k, batch=batch)
    a, b = host(C1).astype(np.float64), host(C2).astype(np.float64)
    assert np.abs(a - b).max() <= 4 * 2.0 ** -11 * np.abs(b).max()


# ---------------------------------------------------------------------------------------------
# full-size, size-independent properties on BASELINE.json's ResNet-50 shapes (b = 32)
# ---------------------------------------------------------------------------------------------
RESNET50_UNIQUE = [(12544, 64, 147), (12544, 64, 64), (12544, 64, 576), (12544, 256, 64), (12544, 64, 256),
                   (12544, 128, 256), (3136, 128, 1152), (3136, 512, 128), (3136, 128, 512), (3136, 256, 512),
                   (784, 256, 2304), (784, 1024, 256), (784, 256, 1024), (784, 512, 1024), (196, 512, 4608),
                   (196, 2048, 512), (196, 512, 2048)]


@pytest.mark.parametrize("shape", RESNET50_UNIQUE, ids=lambda s: "x".join(map(str, s)))
def test_full_size_properties_resnet50(gpu, orc, shape):
    """At b = 32 the oracle is too slow to run in full, so check properties that do not depend on size:
    prune is idempotent and passes the check, decompress(compress(A)) == prune(A) bit for bit,
    spmma is linear in B (spmma(A, 2B) == 2 * spmma(A, B) exactly in fp16 for power-of-two scaling),
    spmma == dense gemm of the pruned matrix, and one sampled batch matches the oracle."""
    import torch
    m, n, k = shape
    batch = 32
    dA = torch.empty(batch * m * k, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dA, 0x5EED + m + k, 0.0, 1.0)
    dB = torch.empty(k * n, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dB, 0xB0B + n, 0.0, 1.0)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    P = dA.clone()
    gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
    valid = torch.ones(1, dtype=torch.int32, device="cuda")
    gpu.prune24_check(P, batch * m, k, k, valid)
    assert int(valid.item()) == 0
    P2 = P.clone()
    gpu.prune24(P2, P2, batch * m, k, k, gpu.PRUNE_STRIP)
    assert torch.equal(P.view(torch.int16), P2.view(torch.int16)), "prune not idempotent"
    D = torch.full_like(P, 7.0)
    gpu.decompress24(blob, m, k, k, batch, m * k, D)
    assert torch.equal(D.view(torch.int16), P.view(torch.int16)), "decompress(compress(A)) != prune(A)"
    exactly_half = (P != 0).sum().item() <= batch * m * ((k + 3) // 4) * 2
    assert exactly_half
    C = torch.empty(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, C, m, n, k, batch)
    C2 = torch.empty_like(C)
    gpu.spmma(blob, dB * 2, C2, m, n, k, batch)
    assert torch.equal((C * 2).view(torch.int16), C2.view(torch.int16)), "spmma not linear in B"
    if n % 8 == 0 and (k % 64 == 0 or n <= 128):  # the fused kernels (direct / wide / A-stationary / span by shape) at full size, b = 32: same bits
        C3 = torch.full_like(C, 3.0)
        gpu.spmma_fused(dA, dB, C3, m, n, k, batch=batch)
        assert torch.equal(C3.view(torch.int16), C.view(torch.int16)), "fused != compress + spmma at full size"
    Cd = torch.empty_like(C)
    gpu.gemm_rowmajor(P, dB, Cd, m, n, k, batch=batch)
    assert (C.float() - Cd.float()).abs().max().item() <= 4 * 2.0 ** -11 * Cd.float().abs().max().item()
    # one sampled batch against the oracle (rows of the last batch)
    b = batch - 1
    rows = min(m, 64)
    Ah = host(dA[b * m * k: b * m * k + rows * k])
    ob = orc.compress24(bits(Ah), rows, k, k)
    Cref = np.zeros(rows * n, dtype=np.uint16)
    orc.spmma(ob, bits(host(dB)), Cref, rows, n, k)
    got = host(C[b * m * n: b * m * n + rows * n])
    scale = (np.abs(Ah.astype(np.float64)).reshape(rows, k) @ np.abs(host(dB).astype(np.float64)).reshape(k, n)).reshape(-1)
    check_close(got, Cref.view(np.float16), scale, FP16_TOL, f"sampled batch {shape}", k)


@pytest.mark.parametrize("shape", [(196, 1, 9, 64), (49, 1, 25, 96), (784, 1, 9, 33), (100, 3, 18, 8), (64, 7, 64, 4), (3136, 1, 9, 512), (8, 1, 8, 1)],
                         ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
def test_fused_thin_vs_oracle(gpu, orc, shape, bf, ab):
    """The THIN form of the fused kernel (round 5, spmma_f16_thin.hip): n < 8 output columns, k <= 64 -- the depthwise convolutions of
    the model zoo as im2col products (n = 1, k = 9 / 25, thousands of batch entries) -- on the vector ALUs.  Against the ORACLE's
    compress -> spmma inside the tight bound (one rounding + k fp32 accumulation steps), ties and ragged last strips included; and
    against the staged pair on the GPU, which adds the same products in the matrix instruction's order: within one rounding of it."""
    import torch
    m, n, k, batch = shape
    alpha, beta = ab
    assert gpu.spmma_fused_form(m, n, k, batch=batch, beta=beta) == "thin", f"{shape} reaches another form"
    rng = np.random.default_rng(m + 5 * n + 7 * k + batch + 3 * bf)
    kind = "ties" if k == 25 else "uniform"
    if bf:
        A, Bm, C0 = bf16_bits(rng, batch * m * k, kind), bf16_bits(rng, k * n), bf16_bits(rng, batch * m * n)
        dA, dB, mk = bf16_dev(A), bf16_dev(Bm), bf16_dev
    else:
        A, Bm, C0 = bits(rand(rng, batch * m * k, np.float16, kind)), bits(rand(rng, k * n, np.float16)), bits(rand(rng, batch * m * n, np.float16))
        mk = lambda x: torch.from_numpy(x.view(np.int16)).cuda().view(torch.float16)
        dA, dB = mk(A), mk(Bm)
    C1 = mk(C0.copy())
    gpu.spmma_fused(dA, dB, C1, m, n, k, batch=batch, alpha=alpha, beta=beta)
    assert torch.equal(dA.view(torch.int16), mk(A).view(torch.int16)), "A was modified"
    ob = orc.compress24(A, m, k, k, batch)
    Cref = C0.copy()
    if bf:
        orc.spmma(ob, Bm, Cref, m, n, k, batch, 0, alpha=alpha, beta=beta, bf16=True)
        pruned = orc.prune24(A, batch * m, k, k, orc.STRIP, bf16=True)
        scale = abs(alpha) * (np.abs(bf16_f64(pruned)).reshape(batch * m, k) @ np.abs(bf16_f64(Bm)).reshape(k, n)).reshape(-1) + abs(beta) * np.abs(bf16_f64(C0))
        check_close(bf16_f64(bf16_host(C1)), bf16_f64(Cref), scale, FP16_TOL, f"thin bf16 {shape}", k, "bf16")
    else:
        orc.spmma(ob, Bm, Cref, m, n, k, batch, 0, alpha=alpha, beta=beta)
        P = np.abs(orc.decompress24(ob, m, k, k, np.uint16, batch=batch).view(np.float16).astype(np.float64)).reshape(batch * m, k)
        scale = abs(alpha) * (P @ np.abs(Bm.view(np.float16).astype(np.float64)).reshape(k, n)).reshape(-1) + abs(beta) * np.abs(C0.view(np.float16).astype(np.float64))
        check_close(host(C1), Cref.view(np.float16), scale, FP16_TOL, f"thin {shape}", k)
    # the staged pair on the GPU: the same products, another order of fp32 additions
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    C2 = mk(C0.copy())
    gpu.spmma(blob, dB, C2, m, n, k, batch, 0, alpha=alpha, beta=beta)
    d = (C1.double() - C2.double()).abs()
    lim = (2.0 ** -7 if bf else 2.0 ** -10) * torch.maximum(C1.double().abs(), C2.double().abs()) + 2.0 * k * 2.0 ** -24 * torch.from_numpy(scale).cuda() + 1e-7
    assert bool((d <= lim).all().item()), "thin form and staged pair differ by more than a rounding"


ZOO_TABLES = ["mobilenetv2", "mobilenetv3_small", "mobilenetv3_large", "densenet161", "densenet201"]


@pytest.mark.parametrize("table", ZOO_TABLES)
def test_model_zoo_tables_full_size(gpu, orc, table):
    """The rest of the reference's model zoo (datasets/get_shapes.py:87-98; tables written by datasets/gen_shapes.py): EVERY unique
    (m, n, k, b) of the table at its full size -- depthwise layers as b x groups products with n = 1 and k = 9 / 25, ragged k (16, 24,
    27, 40, 72, 147, ...), b up to 30 720 -- through prune (STRIP: idempotent, passes the check), compress / decompress (== prune,
    bit for bit), the staged 2:4 matmul (linear in B, one sampled batch entry against the ORACLE inside the tight bound) and, where
    the fused kernels take the shape (n % 8 == 0 and whole 64-deep stages, or the span form), the fused kernel: same bits as the
    staged pair.  Which shapes leave the fused kernels is written to gpurun_out/zoo_<table>_kernels.txt (profiles/ keeps a copy)."""
    import csv
    import os
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(open(os.path.join(root, "datasets", table + ".csv"))))[1:] if r]
    uniq = list(dict.fromkeys(rows))
    report = []
    for (m, n, k, batch) in uniq:
        dA = torch.empty(batch * m * k, dtype=torch.float16, device="cuda")
        gpu.fill_uniform(dA, 0x200 + m + 3 * k, 0.0, 1.0)     # (positive data, as the ResNet-50 test: 2 x C is then exact in fp16 -- no
        dB = torch.empty(k * n, dtype=torch.float16, device="cuda")   #  cancellation into the subnormal range)
        gpu.fill_uniform(dB, 0x300 + n, 0.0, 1.0)
        blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
        gpu.compress24(dA, m, k, k, batch, m * k, blob)
        P = dA.clone()
        gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
        valid = torch.ones(1, dtype=torch.int32, device="cuda")
        gpu.prune24_check(P, batch * m, k, k, valid)
        assert int(valid.item()) == 0, f"{table} {(m, n, k, batch)}: pruned operand fails the check"
        D = torch.full_like(P, 7.0)
        gpu.decompress24(blob, m, k, k, batch, m * k, D)
        assert torch.equal(D.view(torch.int16), P.view(torch.int16)), f"{table} {(m, n, k, batch)}: decompress(compress(A)) != prune(A)"
        del D
        C = torch.empty(batch * m * n, dtype=torch.float16, device="cuda")
        gpu.spmma(blob, dB, C, m, n, k, batch)
        C2 = torch.empty_like(C)
        gpu.spmma(blob, dB * 2, C2, m, n, k, batch)
        assert torch.equal((C * 2).view(torch.int16), C2.view(torch.int16)), f"{table} {(m, n, k, batch)}: spmma not linear in B"
        del C2
        C3 = torch.full_like(C, 3.0)
        fused = "fused"
        try:
            gpu.spmma_fused(dA, dB, C3, m, n, k, batch=batch)
        except gpu.SparsifymeError as e:
            assert "status 2" in str(e), str(e)     # NOT_SUPPORTED: the shape stays on the staged pair
            fused = "staged only (n %% 8 = %d, k %% 64 = %d)" % (n % 8, k % 64)
        if fused == "fused" and n < 8 and k <= 64:
            fused = "fused (thin form)"   # vector-ALU kernel: the staged pair's products in another order of fp32 additions
            lim = 2.0 ** -10 * torch.maximum(C3.float().abs(), C.float().abs()) + 2.0 ** -20 * k
            assert bool(((C3.float() - C.float()).abs() <= lim).all().item()), f"{table} {(m, n, k, batch)}: thin form differs from compress + spmma by more than a rounding"
        elif fused == "fused":
            assert torch.equal(C3.view(torch.int16), C.view(torch.int16)), f"{table} {(m, n, k, batch)}: fused != compress + spmma"
        else:
            assert n % 8 != 0 or (k % 64 != 0 and (n > 128 or (batch * m * k * 2) % 16 != 0 or 128 * k * 2 + 1152 + (k + 63) // 64 * 64 * (64 if n <= 64 else 128) * 2 > 160 * 1024)), \
                f"{table} {(m, n, k, batch)}: a shape the fused kernels document as theirs was declined"
        del C3
        report.append("%6d %5d %5d %6d  %s" % (m, n, k, batch, fused))
        # one sampled batch entry against the oracle
        b = batch - 1
        nr = min(m, 64)
        Ah = host(dA[b * m * k: b * m * k + nr * k])
        ob = orc.compress24(bits(Ah), nr, k, k)
        Cref = np.zeros(nr * n, dtype=np.uint16)
        orc.spmma(ob, bits(host(dB)), Cref, nr, n, k)
        got = host(C[b * m * n: b * m * n + nr * n])
        Pm = np.abs(orc.decompress24(ob, nr, k, k, np.uint16).view(np.float16).astype(np.float64)).reshape(nr, k)
        scale = (Pm @ np.abs(host(dB).astype(np.float64)).reshape(k, n)).reshape(-1)
        check_close(got, Cref.view(np.float16), scale, FP16_TOL, f"{table} sampled batch {(m, n, k, batch)}", k)
        del dA, dB, blob, P, C
    try:
        d = os.path.join(root, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "zoo_%s_kernels.txt" % table), "w") as fh:
            fh.write("# %s: %d layers, %d unique shapes; which 2:4 path each takes (tests/test_gpu_parity.py::test_model_zoo_tables_full_size)\n" % (table, len(rows), len(uniq)))
            fh.write("#    m     n     k      b  path\n" + "\n".join(report) + "\n")
            fh.write("# %d of %d unique shapes run the fused kernels\n" % (sum(1 for r in report if "  fused" in r), len(uniq)))
    except OSError:
        pass


PRUNE_SPMMA_SHAPES = [(128, 64, 64, 1), (196, 128, 256, 2), (132, 72, 192, 3), (4, 8, 64, 1), (260, 128, 128, 2), (3136, 128, 512, 2), (12544, 64, 576, 1),
                      # round 6: everything the exact fused kernels take runs as prune-in-place pass + fused kernel on the pruned operand (no blob):
                      # n > 128 (direct two-tile / big / wide / astat forms), ragged k (span form), m % 4 != 0 (per-batch tiles)
                      (196, 256, 256, 2), (196, 512, 128, 2), (132, 264, 192, 3), (784, 256, 1024, 2), (196, 2048, 512, 1), (196, 512, 2048, 2), (12544, 256, 64, 1),
                      (196, 64, 147, 2), (130, 256, 64, 2), (130, 64, 64, 3)]


@pytest.mark.parametrize("alg", [0, 1], ids=["tile", "strip"])
@pytest.mark.parametrize("shape", PRUNE_SPMMA_SHAPES, ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["uniform", "ties"])
def test_prune_spmma_one_kernel(gpu, orc, alg, shape, bf, kind):
    """sm_prune24_spmma_* -- sparsifyme::spmma()'s whole sequence (spmma.hxx:82-113: prune in place, check, compress, multiply) as
    one kernel with no blob: the pruned operand it writes is bit-identical to sm_prune24_* (itself held against the oracle,
    test_prune24 / test_prune24_bf16_vs_oracle; on the small shapes also against the oracle here), C is bit-identical to
    sm_spmma(sm_compress24(pruned)), the flag is clear and the independent sm_prune24_check agrees; in place and out of place;
    alpha / beta."""
    import torch
    m, n, k, batch = shape
    tdt = torch.bfloat16 if bf else torch.float16
    rng = np.random.default_rng(m * 7 + n * 3 + k + batch + alg)
    if kind == "ties":
        Ah = rng.integers(-3, 4, batch * m * k).astype(np.float32)
    else:
        Ah = rng.uniform(-1, 1, batch * m * k).astype(np.float32)
    dA = torch.from_numpy(Ah).cuda().to(tdt)
    dB = torch.empty(k * n, dtype=tdt, device="cuda")
    gpu.fill_uniform(dB, 0xB1 + n, -1.0, 1.0)
    C0 = torch.empty(batch * m * n, dtype=tdt, device="cuda")
    gpu.fill_uniform(C0, 0xC1 + m, -1.0, 1.0)
    # the staged reference on the GPU: prune -> compress -> spmma
    P = dA.clone()
    if m % 4 == 0 or alg == 1:
        gpu.prune24(P, P, batch * m, k, k, alg)
    else:  # a 4 x 4 tile never spans two batch matrices: per matrix
        for b_ in range(batch):
            gpu.prune24(P[b_ * m * k:(b_ + 1) * m * k], P[b_ * m * k:(b_ + 1) * m * k], m, k, k, alg)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(P, m, k, k, batch, m * k, blob)
    for (alpha, beta, inplace) in [(1.0, 0.0, False), (0.5, -2.0, True)]:
        Cref = C0.clone()
        gpu.spmma(blob, dB, Cref, m, n, k, batch, alpha=alpha, beta=beta)
        Ain = dA.clone()
        Aout = Ain if inplace else torch.full_like(Ain, 7.0)
        C = C0.clone()
        valid = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        gpu.prune24_spmma(Ain, Aout, dB, C, m, n, k, batch=batch, alg=alg, d_valid=valid, alpha=alpha, beta=beta)
        assert torch.equal(Aout.view(torch.int16), P.view(torch.int16)), "pruned operand differs from sm_prune24"
        assert torch.equal(C.view(torch.int16), Cref.view(torch.int16)), "C differs from spmma(compress(prune(A)))"
        assert int(valid.item()) == 0
        if not inplace:
            assert torch.equal(Ain.view(torch.int16), dA.view(torch.int16)), "A_in was modified by the out-of-place form"
        chk = torch.ones(1, dtype=torch.int32, device="cuda")
        gpu.prune24_check(Aout, batch * m, k, k, chk)
        assert int(chk.item()) == 0
    if batch * m * k <= 200000 and not bf:  # small: the pruned operand AND the product against the oracle directly
        oalg = orc.TILE if alg == 0 else orc.STRIP
        if m % 4 == 0 or alg == 1:
            want = orc.prune24(bits(host(dA)), batch * m, k, k, oalg)
        else:
            hA = bits(host(dA))
            want = np.concatenate([orc.prune24(hA[b_ * m * k:(b_ + 1) * m * k], m, k, k, oalg) for b_ in range(batch)])
        assert np.array_equal(bits(host(P)), want)
        Cx = torch.empty(batch * m * n, dtype=tdt, device="cuda")
        gpu.prune24_spmma(dA.clone(), torch.empty_like(dA), dB, Cx, m, n, k, batch=batch, alg=alg)
        ob = orc.compress24(want, m, k, k, batch)
        Cor = np.zeros(batch * m * n, dtype=np.uint16)
        orc.spmma(ob, bits(host(dB)), Cor, m, n, k, batch, 0)
        Pm = np.abs(want.view(np.float16).astype(np.float64)).reshape(batch, m, k)
        Bm = np.abs(host(dB).astype(np.float64)).reshape(k, n)
        scale = np.stack([Pm[b_] @ Bm for b_ in range(batch)]).reshape(-1)
        check_close(host(Cx), Cor.view(np.float16), scale, FP16_TOL, f"prune24_spmma {shape} alg {alg} vs oracle", k)


def _resnet50_unique():
    import csv
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "datasets", "resnet50.csv"), newline="") as fh:
        rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(fh))[1:] if r]
    return sorted(set(rows))


@pytest.mark.parametrize("shape", _resnet50_unique(), ids=lambda s_: "x".join(map(str, s_)))
def test_prune_spmma_takes_every_resnet50_layer_full_size(gpu, shape):
    """sm_prune24_spmma_f16 -- TILE prune IN PLACE + flag + multiply, no blob -- on each of the 17 unique ResNet-50
    shapes at b = 32: dA and dC bit-identical to the staged sequence (sm_prune24 TILE, sm_compress24, sm_spmma), flag clear; and the flag
    of the independent check rises on the unpruned operand (flag semantics)."""
    import torch
    m, n, k, batch = shape
    dA = torch.empty(batch * m * k, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dA, 0xA6 + m + k, -1.0, 1.0)
    dB = torch.empty(k * n, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dB, 0xB6 + n, -1.0, 1.0)
    chk = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu.prune24_check(dA, batch * m, k, k, chk)
    assert int(chk.item()) != 0, "a dense random operand must fail the 2:4 check"
    P = dA.clone()
    gpu.prune24(P, P, batch * m, k, k, 0)      # m % 4 == 0 on every ResNet-50 layer: the batch is one tall matrix
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(P, m, k, k, batch, m * k, blob)
    Cref = torch.empty(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, Cref, m, n, k, batch)
    del blob
    C = torch.full_like(Cref, 3.0)
    valid = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    rc = gpu.prune24_spmma(dA, dA, dB, C, m, n, k, batch=batch, alg=0, d_valid=valid, check=False)
    assert rc == 0, "sm_prune24_spmma_f16 must take every ResNet-50 layer"
    assert int(valid.item()) == 0
    assert torch.equal(dA.view(torch.int16), P.view(torch.int16)), "dA (pruned in place) differs from sm_prune24 TILE"
    assert torch.equal(C.view(torch.int16), Cref.view(torch.int16)), "dC differs from spmma(compress(prune(A)))"


def test_prune_spmma_rejects_what_it_cannot_take(gpu):
    import torch
    A = torch.zeros(200 * 256, dtype=torch.float16, device="cuda")
    B = torch.zeros(256 * 256, dtype=torch.float16, device="cuda")
    C = torch.zeros(200 * 256, dtype=torch.float16, device="cuda")
    NS = gpu.STATUS_NOT_SUPPORTED
    # (round 6: n > 128, ragged k and m % 4 != 0 are TAKEN now -- prune pass + exact fused kernel, test_prune_spmma_one_kernel)
    snap = A.clone()
    assert gpu.prune24_spmma(A, A, B, C, 196, 60, 64, check=False) == NS          # n % 8 != 0: no exact fused form
    assert gpu.prune24_spmma(A, A, B, C, 196, 4, 64, check=False) == NS           # thin shapes: the fused form there is not the staged pair's bits
    assert gpu.prune24_spmma(A[4:], A[4:], B, C, 196, 256, 64, check=False) == NS  # 8-byte aligned A
    assert torch.equal(A, snap), "a refused call must leave A untouched"
    with pytest.raises(gpu.SparsifymeError):
        gpu.prune24_spmma(A, A, B, C, 196, 64, 64, alg=7)


def _resnet50_groups():
    """(m, n, k, count) of datasets/resnet50.csv: the grouped launches of bench.py's timed step (one grid per shape)"""
    import collections
    import csv
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "datasets", "resnet50.csv"), newline="") as fh:
        rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(fh))[1:] if r]
    cnt = collections.Counter(rows)
    return [(m, n, k, c) for (m, n, k, b), c in cnt.items()]


@pytest.mark.parametrize("group", _resnet50_groups(), ids=lambda g: "%dx%dx%d_x%d" % g)
def test_bench_step_launches_equal_staged_pair(gpu, group):
    """What bench.py TIMES, checked: every shape of the headline table as the grouped launch the step makes -- the table's own
    instance count, b = 32, through sm_spmma_fused_f16_grouped (direct / big / wide / persistent wide / A-stationary / span by
    shape and group size) -- against sm_compress24_f16 + sm_spmma_f16 on the same operands, bit for bit, instance by instance
    (the b = 32 span launch and the 3-6-instance grouped grids were timed but never parity-checked)."""
    import torch
    m, n, k, count = group
    batch = 32
    As, Bs, Cs = [], [], []
    for i in range(count):
        A = torch.empty(batch * m * k, dtype=torch.float16, device="cuda")
        gpu.fill_uniform(A, 0xA000 + 17 * i + m + k, -1.0, 1.0)
        B = torch.empty(k * n, dtype=torch.float16, device="cuda")
        gpu.fill_uniform(B, 0xB000 + 13 * i + n, -1.0, 1.0)
        As.append(A)
        Bs.append(B)
        Cs.append(torch.full((batch * m * n,), float("nan"), dtype=torch.float16, device="cuda"))
    gpu.spmma_fused_grouped(As, Bs, Cs, m, n, k, batch=batch)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    Cref = torch.empty(batch * m * n, dtype=torch.float16, device="cuda")
    for i in range(count):
        gpu.compress24(As[i], m, k, k, batch, m * k, blob)
        gpu.spmma(blob, Bs[i], Cref, m, n, k, batch)
        assert torch.equal(Cs[i].view(torch.int16), Cref.view(torch.int16)), f"grouped fused launch, instance {i} of {count}: C differs from compress + spmma"


# ---------------------------------------------------------------------------------------------
# fp32 / fp64 kernels and the unstructured SpMM entry points
# ---------------------------------------------------------------------------------------------
F32_SHAPES = [(128, 64, 64, 1), (196, 512, 256, 2), (130, 72, 200, 1), (512, 512, 512, 1), (17, 9, 5, 2), (300, 136, 147, 2)]


@pytest.mark.parametrize("shape", F32_SHAPES)
def test_gemm_rowmajor_f32_vs_oracle(gpu, orc, shape):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + n * 3 + k * 7)
    A, B = rand(rng, batch * m * k, np.float32), rand(rng, k * n, np.float32)
    C = torch.zeros(batch * m * n, dtype=torch.float32, device="cuda")
    gpu.gemm_rowmajor(to_dev(A), to_dev(B), C, m, n, k, batch=batch)
    Cref = np.zeros(batch * m * n, dtype=np.float32)
    orc.gemm_rowmajor(A, B, Cref, m, n, k, batch=batch)
    scale = (np.abs(A.astype(np.float64)).reshape(batch * m, k) @ np.abs(B.astype(np.float64)).reshape(k, n)).reshape(-1)
    check_close(host(C), Cref, scale, FP32_TOL, f"gemm_rowmajor_f32 {shape}", k, "f32")
    # the f32 MFMA is an exact fmaf chain: far tighter than the 1e-3 the metric asks for
    check_close(host(C), Cref, scale, 1e-5, f"gemm_rowmajor_f32 tight {shape}", k, "f32")


@pytest.mark.parametrize("shape", F32_SHAPES)
def test_spmma_f32_vs_oracle(gpu, orc, shape):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m * 5 + n + k)
    A, B = rand(rng, batch * m * k, np.float32), rand(rng, k * n, np.float32)
    blob = torch.empty(gpu.compress24_size(m, k, 4, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(to_dev(A), m, k, k, batch, m * k, blob)
    ob = orc.compress24(bits(A), m, k, k, batch)
    assert np.array_equal(host(blob), ob)
    C = torch.zeros(batch * m * n, dtype=torch.float32, device="cuda")
    gpu.spmma(blob, to_dev(B), C, m, n, k, batch, 0)
    Cref = np.zeros(batch * m * n, dtype=np.float32)
    orc.spmma(ob, B, Cref, m, n, k, batch, 0)
    scale = (np.abs(A.astype(np.float64)).reshape(batch * m, k) @ np.abs(B.astype(np.float64)).reshape(k, n)).reshape(-1)
    check_close(host(C), Cref, scale, FP32_TOL, f"spmma_f32 {shape}", k, "f32")


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 512, 256, 2), (130, 72, 224, 1), (512, 512, 512, 1), (33, 12, 32, 3), (300, 136, 160, 2),
                                   (40, 200, 96, 1)])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
def test_spmma_fused_f32(gpu, orc, shape, ab):
    """sm_spmma_fused_f32 (STRIP rule on the A fragments in the dense fp32 MFMA kernel's registers): bit-identical to the
    dense kernel on the pruned operand, within the tight bound of the oracle's compress -> spmma; ties and specials."""
    import torch
    m, n, k, batch = shape
    alpha, beta = ab
    rng = np.random.default_rng(m * 3 + n + k * 7)
    A = rand(rng, batch * m * k, np.float32, "ties" if m % 2 else "uniform")
    if m == 196:
        A[:8] = np.array([1.0, np.nan, np.inf, 2.0, -0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    B, C0 = rand(rng, k * n, np.float32), rand(rng, batch * m * n, np.float32)
    dA, dB = to_dev(A), to_dev(B)
    Cf, Cd = to_dev(C0.copy()), to_dev(C0.copy())
    gpu.spmma_fused(dA, dB, Cf, m, n, k, batch=batch, alpha=alpha, beta=beta)
    P = dA.clone()
    gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
    gpu.gemm_rowmajor(P, dB, Cd, m, n, k, batch=batch, alpha=alpha, beta=beta)
    assert np.array_equal(bits(host(Cf)), bits(host(Cd))), "fused fp32 differs from the dense kernel on the pruned operand"
    if m != 196:   # (the specials row multiplies NaN / inf: compared bit for bit above only)
        ob = orc.compress24(bits(A), m, k, k, batch)
        Cref = C0.copy()
        orc.spmma(ob, B, Cref, m, n, k, batch, 0, alpha=alpha, beta=beta)
        Pm = np.abs(host(P).astype(np.float64)).reshape(batch * m, k)
        scale = abs(alpha) * (Pm @ np.abs(B.astype(np.float64)).reshape(k, n)).reshape(-1) + abs(beta) * np.abs(C0.astype(np.float64))
        check_close(host(Cf), Cref, scale, FP32_TOL, f"spmma_fused_f32 {shape}", k, "f32")


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 128, 256, 2), (132, 72, 192, 3), (260, 256, 128, 2), (132, 200, 192, 3), (100, 512, 320, 1),
                                   (3136, 128, 576, 2), (784, 256, 1152, 2), (12544, 64, 576, 1), (300, 64, 147, 2), (130, 72, 100, 1), (128, 64, 72, 1),
                                   (3136, 64, 147, 4)], ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("planes", [3, 2])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
@pytest.mark.parametrize("kind", ["uniform", "ties"])
def test_spmma_f32_split(gpu, orc, shape, planes, ab, kind):
    """sm_spmma_fused_f32_split -- the fp32 2:4 product on v_smfmac_f32_16x16x64_bf16 through exact bfloat16 splits.  On small-integer
    data every piece product is exact, so C must EQUAL the exact fp32 kernel's bit for bit (same mask, ties included); on U(-1, 1)
    data the error against the fp64 product of the STRIP-pruned operand stays inside SPLIT_TOL * sum|a||b| + the fp32 accumulation
    bound -- three (planes = 2) to five (planes = 3) orders of magnitude inside north_star's 1e-3."""
    import torch
    m, n, k, batch = shape
    alpha, beta = ab
    rng = np.random.default_rng(m + 3 * n + 5 * k + planes)
    A = rand(rng, batch * m * k, np.float32, kind)
    B = rand(rng, k * n, np.float32, kind)
    C0 = rand(rng, batch * m * n, np.float32, kind)
    dA, dB = to_dev(A), to_dev(B)
    ws = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k, planes=planes), dtype=torch.uint8, device="cuda")
    Cs, Ce = to_dev(C0.copy()), to_dev(C0.copy())
    gpu.spmma_fused_f32_split(dA, dB, Cs, m, n, k, ws, batch=batch, planes=planes, alpha=alpha, beta=beta)
    assert torch.equal(dA.view(torch.int32), to_dev(A).view(torch.int32)), "A was modified"
    P = dA.clone()
    gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
    if k % 32 == 0:
        gpu.spmma_fused(dA, dB, Ce, m, n, k, batch=batch, alpha=alpha, beta=beta)
    else:   # ragged k (the span form): the exact fused kernel does not take it; the dense fp32 kernel on the pruned operand is the same product
        gpu.gemm_rowmajor(P, dB, Ce, m, n, k, batch=batch, alpha=alpha, beta=beta)
    #  mask and reference from the ORACLE, not from the HIP prune: the oracle's STRIP-pruned operand must be what the
    # HIP prune wrote (bit for bit) and is what the fp64 reference below multiplies; the oracle's own product (compress -> sm_spmma_f32_ref, fp64
    # accumulation, rounded to fp32) is held against the split form at north_star's tolerance as well
    Po = orc.prune24(A.view(np.uint32), batch * m, k, k, orc.STRIP)
    assert np.array_equal(host(P).view(np.uint32), Po), "HIP STRIP prune differs from the oracle's"
    if kind == "ties" and beta == 0.0:
        assert torch.equal(Cs.view(torch.int32), Ce.view(torch.int32)), "exact data: the split form must equal the fp32 kernel bit for bit"
        Co = np.zeros(batch * m * n, dtype=np.float32)
        orc.spmma(orc.compress24(Po, m, k, k, batch), B, Co, m, n, k, batch, 0, alpha=alpha, beta=0.0)
        assert np.array_equal(host(Cs), Co), "exact data: the split form must equal the oracle's product"
        return
    P64 = Po.view(np.float32).astype(np.float64).reshape(batch * m, k)
    B64 = B.astype(np.float64).reshape(k, n)
    ref = alpha * (P64 @ B64).reshape(-1) + beta * C0.astype(np.float64)
    Co = C0.copy()
    orc.spmma(orc.compress24(Po, m, k, k, batch), B, Co, m, n, k, batch, 0, alpha=alpha, beta=beta)
    sc_ = abs(alpha) * (np.abs(P64) @ np.abs(B64)).reshape(-1) + abs(beta) * np.abs(C0.astype(np.float64))
    assert not (np.abs(host(Cs).astype(np.float64) - Co.astype(np.float64)) > FP32_TOL * np.maximum(sc_, 1e-30)).any(), "split form vs orc.spmma outside 1e-3"
    scale = abs(alpha) * (np.abs(P64) @ np.abs(B64)).reshape(-1) + abs(beta) * np.abs(C0.astype(np.float64))
    err = np.abs(host(Cs).astype(np.float64) - ref)
    bound = split_bound(planes, k, scale, ref)
    ratio = float((err / bound).max())
    assert ratio <= 1.0, f"split planes={planes} {shape}: max err / bound = {ratio:.3f} (max err {err.max():.3e})"
    assert not (err > FP32_TOL * np.maximum(scale, 1e-30)).any()


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 128, 256, 2), (260, 256, 128, 2), (132, 200, 192, 3), (100, 512, 320, 1), (3136, 64, 576, 1),
                                   (300, 64, 147, 2), (130, 72, 100, 1)], ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("planes", [3, 2])
@pytest.mark.parametrize("kind", ["uniform", "ties"])
def test_gemm_f32_split_dense(gpu, orc, shape, planes, kind):
    """sm_gemm_rowmajor_f32_split: the dense product by the same bfloat16 pieces (v_mfma_f32_16x16x32_bf16).  Exact data: equal to
    sm_gemm_rowmajor_f32 bit for bit; U(-1, 1): inside SPLIT_TOL * sum|a||b| + the fp32 accumulation bound of the fp64 product."""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + n + k + planes)
    A, B = rand(rng, batch * m * k, np.float32, kind), rand(rng, k * n, np.float32, kind)
    dA, dB = to_dev(A), to_dev(B)
    ws = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k, planes=planes), dtype=torch.uint8, device="cuda")
    Cs = torch.zeros(batch * m * n, dtype=torch.float32, device="cuda")
    Ce = torch.zeros(batch * m * n, dtype=torch.float32, device="cuda")
    gpu.spmma_fused_f32_split(dA, dB, Cs, m, n, k, ws, batch=batch, planes=planes, dense=True)
    gpu.gemm_rowmajor(dA, dB, Ce, m, n, k, batch=batch)
    #  ... and against the ORACLE's dense product (sm_cpu_gemm-free: orc.gemm_rowmajor, fp64 accumulation)
    Co = np.zeros(batch * m * n, dtype=np.float32)
    orc.gemm_rowmajor(A, B, Co, m, n, k, batch=batch)
    if kind == "ties":
        assert torch.equal(Cs.view(torch.int32), Ce.view(torch.int32))
        assert np.array_equal(host(Cs), Co), "exact data: the dense split form must equal the oracle's product"
        return
    sc_ = (np.abs(A.astype(np.float64)).reshape(batch * m, k) @ np.abs(B.astype(np.float64)).reshape(k, n)).reshape(-1)
    assert not (np.abs(host(Cs).astype(np.float64) - Co.astype(np.float64)) > FP32_TOL * np.maximum(sc_, 1e-30)).any(), "dense split form vs oracle outside 1e-3"
    A64, B64 = A.astype(np.float64).reshape(batch * m, k), B.astype(np.float64).reshape(k, n)
    ref, scale = (A64 @ B64).reshape(-1), (np.abs(A64) @ np.abs(B64)).reshape(-1)
    err = np.abs(host(Cs).astype(np.float64) - ref)
    bound = split_bound(planes, k, scale, ref)
    assert float((err / bound).max()) <= 1.0, f"dense split planes={planes} {shape}: max err {err.max():.3e}"


@pytest.mark.parametrize("dense", [False, True], ids=["2to4", "dense"])
@pytest.mark.parametrize("planes", [3, 2])
def test_f32_split_per_batch_b_and_alpha_beta(gpu, dense, planes):
    """The split forms with a B per batch entry (strideB = k * n: what spmma<float> passes, examples/spmma.cu:48-59) and alpha / beta:
    every batch entry equals its own single-matrix call bit for bit, and stays inside the bound of the fp64 product."""
    import torch
    m, n, k, batch = 196, 128, 256, 3
    alpha, beta = 0.5, -2.0
    rng = np.random.default_rng(planes + 10 * dense)
    A, B, C0 = rand(rng, batch * m * k, np.float32), rand(rng, batch * k * n, np.float32), rand(rng, batch * m * n, np.float32)
    dA, dB = to_dev(A), to_dev(B)
    ws = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k, batch=batch, strideB=k * n, planes=planes), dtype=torch.uint8, device="cuda")
    C = to_dev(C0.copy())
    gpu.spmma_fused_f32_split(dA, dB, C, m, n, k, ws, batch=batch, strideB=k * n, planes=planes, alpha=alpha, beta=beta, dense=dense)
    ws1 = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k, planes=planes), dtype=torch.uint8, device="cuda")
    for b in range(batch):
        C1 = to_dev(C0[b * m * n:(b + 1) * m * n].copy())
        gpu.spmma_fused_f32_split(dA[b * m * k:(b + 1) * m * k], dB[b * k * n:(b + 1) * k * n], C1, m, n, k, ws1, planes=planes, alpha=alpha, beta=beta,
                                  dense=dense)
        assert torch.equal(C[b * m * n:(b + 1) * m * n].view(torch.int32), C1.view(torch.int32)), f"batch entry {b} differs from its own call"
    P = dA.clone()
    if not dense:
        gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
    P64 = host(P).astype(np.float64).reshape(batch, m, k)
    B64 = B.astype(np.float64).reshape(batch, k, n)
    ref = alpha * np.einsum("bmk,bkn->bmn", P64, B64).reshape(-1) + beta * C0.astype(np.float64)
    scale = abs(alpha) * np.einsum("bmk,bkn->bmn", np.abs(P64), np.abs(B64)).reshape(-1) + abs(beta) * np.abs(C0.astype(np.float64))
    err = np.abs(host(C).astype(np.float64) - ref)
    bound = split_bound(planes, k, scale, ref)
    assert float((err / bound).max()) <= 1.0


@pytest.mark.parametrize("dense", [False, True], ids=["2to4", "dense"])
@pytest.mark.parametrize("planes", [3, 2])
@pytest.mark.parametrize("k", [64, 192])
def test_f32_split_cols_last_stage_waits_for_its_own_b(gpu, dense, planes, k):
    """The column-loop form (128 < n <= 256) on its LAST K stage: no A(kt + 1) follows B(kt, 1), so the counted wait in front of
    the second 128-column half must drain everything (with vmcnt(SLA) the sweep could read B's second half before
    it landed).  One K stage / three, a B per batch entry large enough (48 - 144 MiB of planes) not to sit in L2, many workgroups,
    small-integer data: C[:, 128:256] must equal the exact fp32 kernel's bit for bit, ten times over."""
    import torch
    m, n, batch = 256, 256, 512
    rng = np.random.default_rng(k + planes + 7 * dense)
    A = rand(rng, batch * m * k, np.float32, "ties")
    B = rand(rng, batch * k * n, np.float32, "ties")
    dA, dB = to_dev(A), to_dev(B)
    P = dA
    if not dense:
        P = dA.clone()
        gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
    Ce = torch.zeros(batch * m * n, dtype=torch.float32, device="cuda")
    for i in range(batch):   # the exact dense fp32 kernel, a B per batch entry
        gpu.gemm_rowmajor(P[i * m * k:(i + 1) * m * k], dB[i * k * n:(i + 1) * k * n], Ce[i * m * n:(i + 1) * m * n], m, n, k)
    ws = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k, batch=batch, strideB=k * n, planes=planes), dtype=torch.uint8, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for rep in range(10):
        C = torch.full((batch * m * n,), float("nan"), dtype=torch.float32, device="cuda")
        flush.fill_(rep)   # push B's planes of the previous repetition out of the caches
        gpu.spmma_fused_f32_split(dA, dB, C, m, n, k, ws, batch=batch, strideB=k * n, planes=planes, dense=dense)
        assert torch.equal(C.view(torch.int32), Ce.view(torch.int32)), f"repetition {rep}: the split form differs from the exact kernel"


@pytest.mark.parametrize("planes", [3, 2])
@pytest.mark.parametrize("shape", [(256, 64, 128, 3, False), (200, 256, 192, 2, True), (130, 512, 64, 2, False), (64, 40, 72, 2, False)])
def test_f32_split_prepared_planes_equal_per_call(gpu, shape, planes):
    """sm_spmma_fused_f32_split_prepare + _prepared (B's planes once, for weights): bit-equal to sm_spmma_fused_f32_split, with B shared and per batch,
    and the prepared call never reads B (it is freed before the call)."""
    import torch
    m, n, k, batch, per_batch = shape
    g = torch.Generator().manual_seed(m * 7 + n + k)
    dA = (torch.rand(batch * m * k, generator=g) * 2 - 1).cuda()
    nb = batch if per_batch else 1
    dB = (torch.rand(nb * k * n, generator=g) * 2 - 1).cuda()
    sB = k * n if per_batch else 0
    ws = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k, batch=batch, strideB=sB, planes=planes), dtype=torch.uint8, device="cuda")
    C0 = torch.full((batch * m * n,), 0.5, device="cuda")
    C1 = C0.clone()
    gpu.spmma_fused_f32_split(dA, dB, C0, m, n, k, ws, batch=batch, strideB=sB, planes=planes, alpha=1.5, beta=-0.25)
    ws.zero_()
    gpu.spmma_fused_f32_split_prepare(dB, n, k, ws, batch=batch, strideB=sB, planes=planes)
    torch.cuda.synchronize()
    del dB
    for _ in range(2):                      # the planes survive a call
        C1.fill_(0.5)
        gpu.spmma_fused_f32_split_prepared(dA, ws, C1, m, n, k, batch=batch, strideB=sB, planes=planes, alpha=1.5, beta=-0.25)
        assert torch.equal(C0, C1)
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fused_f32_split_prepare(dA, n, k, ws[:64], batch=batch, strideB=sB, planes=planes)


def test_spmma_f32_split_edges(gpu):
    """What the split form declines, and what a non-finite operand value does: it stays in the first piece, so the outputs it
    reaches are non-finite (NaN where the exact form may say inf: inf meets a zero low piece) and every other output is untouched."""
    import torch
    m, n, k = 128, 64, 128
    rng = np.random.default_rng(77)
    A, B = rand(rng, m * k, np.float32), rand(rng, k * n, np.float32)
    A[5 * k + 3] = np.inf
    A[5 * k + 2] = 0.5   # so that the inf is kept whatever its neighbours are
    A[9 * k + 64] = np.nan
    dA, dB = to_dev(A), to_dev(B)
    C = torch.zeros(m * n, dtype=torch.float32, device="cuda")
    Ce = torch.zeros(m * n, dtype=torch.float32, device="cuda")
    ws = torch.empty(gpu.spmma_fused_f32_split_workspace(n, k), dtype=torch.uint8, device="cuda")
    gpu.spmma_fused_f32_split(dA, dB, C, m, n, k, ws)
    gpu.spmma_fused(dA, dB, Ce, m, n, k)
    c, ce = host(C).reshape(m, n), host(Ce).reshape(m, n)
    assert not np.isfinite(c[5]).any() and not np.isfinite(c[9]).any()
    rows = [r for r in range(m) if r not in (5, 9)]
    assert np.isfinite(c[rows]).all() and np.allclose(c[rows], ce[rows], rtol=0, atol=1e-4)
    NS, INV = gpu.STATUS_NOT_SUPPORTED, 1
    assert gpu.spmma_fused_f32_split(dA, dB, C, 16, 256, 72, ws, check=False) == NS   # k % 64 != 0 with n > 128: no span form
    assert gpu.spmma_fused_f32_split(dA, dB, C, 64, 12, 64, ws, check=False) == NS    # n % 8 != 0
    small = torch.empty(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fused_f32_split(dA, dB, C, m, n, k, small)                          # workspace too small
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fused_f32_split(dA, dB, C, m, n, k, ws, planes=4)


def test_spmma_fused_f32_rejects_what_it_cannot_take(gpu):
    import torch
    x = torch.zeros(4096, dtype=torch.float32, device="cuda")
    L_ = gpu.lib()
    call = lambda m, n, k, lda: L_.sm_spmma_fused_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), m, n, k, lda, 1, m * lda, 0, m * n, 1.0, 0.0, None)
    assert call(8, 8, 147, 147) == 2      # k % 32 != 0 -> NOT_SUPPORTED (the staged pair serves it)
    assert call(8, 6, 32, 32) == 2        # n % 4 != 0
    assert call(8, 8, 32, 16) == 1        # lda < k -> INVALID_VALUE


@pytest.mark.parametrize("sfx,dtype,tol", [("f32", np.float32, FP32_TOL), ("f64", np.float64, 1e-12)])
@pytest.mark.parametrize("shape", [(128, 64, 64, 2), (196, 512, 100, 2), (130, 72, 200, 3)])
def test_gemm_batched_column_major_f32_f64(gpu, orc, sfx, dtype, tol, shape):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + 2 * n + 3 * k)
    As = [rand(rng, m * k, dtype) for _ in range(batch)]
    Bsh = rand(rng, k * n, dtype)
    dAs, dB = [to_dev(a) for a in As], to_dev(Bsh)
    dCs = [torch.zeros(m * n, dtype=torch_dtype(dtype), device="cuda") for _ in range(batch)]
    ptr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
    gpu.gemm_batched(ptr(dAs), ptr([dB] * batch), ptr(dCs), m, n, k, batch, sfx)
    Cs = [np.zeros(m * n, dtype=dtype) for _ in range(batch)]
    orc.gemm_batched(As, [Bsh] * batch, Cs, m, n, k)
    Bm = np.abs(Bsh.astype(np.float64)).reshape(n, k).T
    for b in range(batch):
        scale = (np.abs(As[b].astype(np.float64)).reshape(k, m).T @ Bm).T.reshape(-1)
        check_close(host(dCs[b]), Cs[b], scale, tol, f"gemm_batched_{sfx} {shape} batch {b}", k, sfx)


@pytest.mark.parametrize("sfx,dtype,tol", [("f16", np.float16, FP16_TOL), ("f32", np.float32, FP32_TOL), ("f64", np.float64, 1e-12)])
@pytest.mark.parametrize("tatb", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape", [(128, 64, 64, 2), (200, 72, 136, 2), (131, 35, 77, 3), (264, 128, 192, 1)])
def test_gemm_batched_transposed_operands(gpu, orc, sfx, dtype, tol, tatb, shape):
    """transpose_a / transpose_b of batched::gemm (gemm.hxx:33-34): the stored operand is read through the leading
    dimensions the reference always passes (lda = m, ldb = k; gemm.hxx:80-81), as the oracle does."""
    import torch
    m, n, k, batch = shape
    ta, tb = tatb
    alpha, beta = 0.75, -0.5
    rng = np.random.default_rng(m + 2 * n + 3 * k + 7 * ta + 11 * tb)
    na = m * m if ta else m * k          # op(A)[i][l] = A[i * lda + l], lda = m >= k
    nb = k * k if tb else k * n          # op(B)[l][j] = B[l * ldb + j], ldb = k >= n
    As = [rand(rng, na, dtype) for _ in range(batch)]
    Bs = [rand(rng, nb, dtype) for _ in range(batch)]
    C0 = [rand(rng, m * n, dtype) for _ in range(batch)]
    dAs, dBs = [to_dev(a) for a in As], [to_dev(b) for b in Bs]
    dCs = [to_dev(c.copy()) for c in C0]
    ptr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")
    gpu.gemm_batched(ptr(dAs), ptr(dBs), ptr(dCs), m, n, k, batch, sfx, alpha, beta, ta=ta, tb=tb)
    view = (lambda x: bits(x)) if sfx == "f16" else (lambda x: x)
    Cs = [view(c.copy()) for c in C0]
    orc.gemm_batched([view(a) for a in As], [view(b) for b in Bs], Cs, m, n, k, alpha, beta, ta=ta, tb=tb)
    for b in range(batch):
        a64, b64 = np.abs(As[b].astype(np.float64)), np.abs(Bs[b].astype(np.float64))
        opA = a64.reshape(m, m)[:, :k] if ta else a64.reshape(k, m).T          # m x k
        opB = b64.reshape(k, k)[:, :n] if tb else b64.reshape(n, k).T          # k x n
        scale = abs(alpha) * (opA @ opB).T.reshape(-1) + abs(beta) * np.abs(C0[b].astype(np.float64))
        got = host(dCs[b])
        want = Cs[b].view(np.float16) if sfx == "f16" else Cs[b]
        check_close(got, want, scale, tol, f"gemm_batched_{sfx} ta={ta} tb={tb} {shape} batch {b}", k, sfx)


def test_gemm_batched_transposed_rejects_short_leading_dimension(gpu):
    """lda = m < k with op(A) = T (or ldb = k < n with op(B) = T) is what the vendor BLAS rejects as an invalid
    leading dimension; the C ABI reports it instead of reading overlapping columns."""
    import torch
    z = torch.zeros(4, dtype=torch.int64, device="cuda")
    L = gpu.lib()
    assert L.sm_gemm_batched_f32(z.data_ptr(), z.data_ptr(), z.data_ptr(), 8, 8, 16, 1, 1, 0, 1.0, 0.0, None) == 1  # SM_STATUS_INVALID_VALUE
    assert L.sm_gemm_batched_f16(z.data_ptr(), z.data_ptr(), z.data_ptr(), 32, 16, 8, 1, 0, 1, 1.0, 0.0, None) == 1  # SM_STATUS_INVALID_VALUE
    assert L.sm_gemm_batched_f64(z.data_ptr(), z.data_ptr(), z.data_ptr(), 8, 8, 8, 1, 2, 0, 1.0, 0.0, None) == 1  # SM_STATUS_INVALID_VALUE


def test_spmm_bell_vs_oracle(gpu, orc):
    import torch
    rng = np.random.default_rng(4)
    for (rows, cols, bs, n) in [(64, 64, 2, 16), (200, 96, 2, 37), (12, 24, 4, 5)]:
        ell_cols = cols // 2
        bcols = ell_cols // bs
        ci = np.stack([np.sort(rng.choice(cols // bs, bcols, replace=False)) for _ in range(rows // bs)]).astype(np.uint64)
        vals = rng.uniform(-1, 1, (rows, ell_cols)).astype(np.float32)
        B = rng.uniform(-1, 1, cols * n).astype(np.float32)
        C0 = rng.uniform(-1, 1, rows * n).astype(np.float32)
        Cref = C0.copy()
        orc.spmm_bell(vals.reshape(-1), ci.reshape(-1), rows, cols, bs, ell_cols, B, Cref, n, 1.5, 0.5)
        dC, dV, dI, dB = to_dev(C0.copy()), to_dev(vals.reshape(-1)), to_dev(ci.reshape(-1).view(np.int64)), to_dev(B)
        rc = gpu.lib().sm_spmm_bell_f32(dV.data_ptr(), dI.data_ptr(), rows, cols, bs, ell_cols, dB.data_ptr(), dC.data_ptr(),
                                        n, 1.5, 0.5, None)
        assert rc == 0
        assert np.allclose(host(dC), Cref, rtol=1e-5, atol=1e-5)
        # workspace form: blocks scattered into a dense A, product on the fp32 matrix cores
        import ctypes
        nb = ctypes.c_size_t(0)
        assert gpu.lib().sm_spmm_bell_workspace_size(rows, cols, ctypes.byref(nb)) == 0
        assert nb.value >= rows * cols * 4
        ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device="cuda")  # stale workspace must not leak
        dC2 = to_dev(C0.copy())
        rc = gpu.lib().sm_spmm_bell_f32_ws(dV.data_ptr(), dI.data_ptr(), rows, cols, bs, ell_cols, dB.data_ptr(),
                                           dC2.data_ptr(), n, 1.5, 0.5, ws.data_ptr(), None)
        assert rc == 0
        assert np.allclose(host(dC2), Cref, rtol=1e-4, atol=1e-4)


def test_spmm_bell_batched_vs_oracle(gpu, orc):
    """sm_spmm_bell_batched_f32: every batch of the reference's spmm() loop in one submission."""
    import ctypes
    import torch
    rng = np.random.default_rng(14)
    rows, cols, bs, n, batch = 136, 160, 2, 70, 5
    ell_cols = cols // 2
    bcols = ell_cols // bs
    B = rng.uniform(-1, 1, cols * n).astype(np.float32)
    dB = to_dev(B)
    keep, refs, dCs = [], [], []
    for b in range(batch):
        ci = np.stack([np.sort(rng.choice(cols // bs, bcols, replace=False)) for _ in range(rows // bs)]).astype(np.uint64)
        vals = rng.uniform(-1, 1, (rows, ell_cols)).astype(np.float32)
        C0 = rng.uniform(-1, 1, rows * n).astype(np.float32)
        Cref = C0.copy()
        orc.spmm_bell(vals.reshape(-1), ci.reshape(-1), rows, cols, bs, ell_cols, B, Cref, n, 0.75, -2.0)
        dV, dI, dC = to_dev(vals.reshape(-1)), to_dev(ci.reshape(-1).view(np.int64)), to_dev(C0.copy())
        keep.append((dV, dI))
        dCs.append(dC)
        refs.append(Cref)
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_bell_batched_workspace_size(rows, cols, batch, ctypes.byref(nb)) == 0
    ws = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device="cuda")
    PtrArr = ctypes.c_void_p * batch
    pv = PtrArr(*[v.data_ptr() for v, _ in keep])
    pi = PtrArr(*[i.data_ptr() for _, i in keep])
    pc = PtrArr(*[c.data_ptr() for c in dCs])
    rc = gpu.lib().sm_spmm_bell_batched_f32(pv, pi, rows, cols, bs, ell_cols, dB.data_ptr(), pc, n, batch, 0.75, -2.0,
                                            ws.data_ptr(), None)
    assert rc == 0
    for dC, Cref in zip(dCs, refs):
        assert np.allclose(host(dC), Cref, rtol=1e-4, atol=1e-4)
    # a missing workspace is an error, not a silent slow path
    assert gpu.lib().sm_spmm_bell_batched_f32(pv, pi, rows, cols, bs, ell_cols, dB.data_ptr(), pc, n, batch, 1.0, 0.0,
                                              None, None) != 0


def test_spmm_coo_vs_oracle(gpu, orc):
    import torch
    rng = np.random.default_rng(6)
    rows, cols, n, batches = 150, 90, 33, 3
    dense = (rng.uniform(0, 1, (rows, cols)) < 0.1)
    r, c = np.nonzero(dense)
    r, c = np.concatenate([r, r[:5]]).astype(np.int32), np.concatenate([c, c[:5]]).astype(np.int32)  # duplicates
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    B = rng.uniform(-1, 1, batches * cols * n).astype(np.float32)
    C0 = rng.uniform(-1, 1, batches * rows * n).astype(np.float32)
    Cref = C0.copy()
    orc.spmm_coo(rows, cols, r.size, n, batches, r, c, v, B, Cref, 2.0, -1.0)
    dC, dr, dc, dv, dB = to_dev(C0.copy()), to_dev(r), to_dev(c), to_dev(v), to_dev(B)
    rc = gpu.lib().sm_spmm_coo_f32(rows, cols, r.size, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(),
                                   dC.data_ptr(), 2.0, -1.0, None)
    assert rc == 0
    assert np.allclose(host(dC), Cref, rtol=1e-4, atol=1e-4)
    # workspace form: row-sorted input -> CSR kernel (no atomics); shuffled input -> atomic fallback; same answer
    import ctypes
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_workspace_size(rows, ctypes.byref(nb)) == 0
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    order = np.lexsort((c, r))
    perm = rng.permutation(r.size)
    for idx in (order, perm):
        dr2, dc2, dv2 = to_dev(r[idx].copy()), to_dev(c[idx].copy()), to_dev(v[idx].copy())
        dC2 = to_dev(C0.copy())
        rc = gpu.lib().sm_spmm_coo_f32_ws(rows, cols, r.size, n, batches, dr2.data_ptr(), dc2.data_ptr(), dv2.data_ptr(),
                                          dB.data_ptr(), dC2.data_ptr(), 2.0, -1.0, ws.data_ptr(), None)
        assert rc == 0
        assert np.allclose(host(dC2), Cref, rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------
# BASELINE.json config 2: the ResNet-18 layer shapes in fp32 at b = 32 (prune + spmma vs gemm), full size
# ---------------------------------------------------------------------------------------------
RESNET18_UNIQUE = [(12544, 64, 147), (12544, 64, 576), (3136, 128, 576), (3136, 128, 1152), (784, 256, 1152),
                   (784, 256, 2304), (196, 512, 2304), (196, 512, 4608)]


@pytest.mark.parametrize("shape", RESNET18_UNIQUE, ids=lambda s: "x".join(map(str, s)))
def test_full_size_properties_resnet18_f32(gpu, orc, shape):
    """Config 2 through the entry points its sweep uses (sm_compress24_f32, sm_spmma_f32, sm_gemm_rowmajor_f32 and the
    reference-layout sm_gemm_batched_f32), at the table's full b = 32: the 2:4 product equals the dense product of the
    pruned operand to fp32 accumulation accuracy everywhere (inputs are U(0,1), so sum|a*b| is the product itself),
    decompress(compress) == prune bit for bit, and sampled rows match the fp64 oracle within the tight bound."""
    import torch
    m, n, k = shape
    batch = 32
    dA = torch.empty(batch * m * k, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dA, 0x18 + m + k, 0.0, 1.0)
    dB = torch.empty(k * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dB, 0xB18 + n, 0.0, 1.0)
    blob = torch.empty(gpu.compress24_size(m, k, 4, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    P = dA.clone()
    gpu.prune24(P, P, batch * m, k, k, gpu.PRUNE_STRIP)
    valid = torch.ones(1, dtype=torch.int32, device="cuda")
    gpu.prune24_check(P, batch * m, k, k, valid)
    assert int(valid.item()) == 0
    D = torch.full_like(P, 7.0)
    gpu.decompress24(blob, m, k, k, batch, m * k, D)
    assert torch.equal(D.view(torch.int32), P.view(torch.int32)), "decompress(compress(A)) != prune(A)"
    del D
    C = torch.full((batch * m * n,), -1.0, dtype=torch.float32, device="cuda")
    gpu.spmma(blob, dB, C, m, n, k, batch)
    Cd = torch.full_like(C, -2.0)
    gpu.gemm_rowmajor(P, dB, Cd, m, n, k, batch=batch)
    if k % 32 == 0:   # the one-kernel fp32 form: the STRIP rule in the registers of the dense MFMA kernel -> the same bits as Cd
        Cf = torch.full_like(C, -4.0)
        gpu.spmma_fused(dA, dB, Cf, m, n, k, batch=batch)
        assert torch.equal(Cf.view(torch.int32), Cd.view(torch.int32)), "sm_spmma_fused_f32 != sm_gemm_rowmajor_f32(prune_strip(A))"
        del Cf
    # same products, fp32 accumulation in two different orders: |C - Cd| <= 2 k u sum|ab| = 2 k u Cd  (u = 2^-24)
    worst = ((C - Cd).abs() / Cd.clamp_min(1e-30)).max().item()
    assert worst <= 2 * k * 2.0 ** -24, f"spmma_f32 vs gemm_f32(prune): {worst:.3e} relative to sum|ab|"
    assert worst <= 1e-5 * max(1.0, k / 80.0)
    # sampled rows of the last batch against the oracle
    b = batch - 1
    rows = min(m, 48)
    Ah = host(dA[b * m * k: b * m * k + rows * k])
    Bh = host(dB)
    ob = orc.compress24(bits(Ah), rows, k, k)
    Cref = np.zeros(rows * n, dtype=np.float32)
    orc.spmma(ob, Bh, Cref, rows, n, k)
    Pm = np.abs(orc.decompress24(ob, rows, k, k, np.uint32).view(np.float32).astype(np.float64)).reshape(rows, k)
    scale = (Pm @ np.abs(Bh.astype(np.float64)).reshape(k, n)).reshape(-1)
    check_close(host(C[b * m * n: b * m * n + rows * n]), Cref, scale, FP32_TOL, f"resnet18 f32 spmma sampled {shape}", k, "f32")
    Cdref = np.zeros(rows * n, dtype=np.float32)
    orc.gemm_rowmajor(host(P[b * m * k: b * m * k + rows * k]), Bh, Cdref, rows, n, k)
    check_close(host(Cd[b * m * n: b * m * n + rows * n]), Cdref, scale, FP32_TOL, f"resnet18 f32 gemm_rm sampled {shape}", k, "f32")
    # (round 6) the DEFAULT fp32 path since this round -- the split form, planes = 3 (spmma_options().f32_planes, bench.py --dtype f32) -- at
    # full size: everywhere within 2^-21 sum|ab| + the accumulation bound of the exact kernel's C, and the sampled rows against the ORACLE
    # (its compress -> sm_spmma_f32_ref product: fp64 accumulation) inside SPLIT_TOL[3] * sum|ab| + the fp32 accumulation bound
    ws = torch.empty(max(16, gpu.spmma_fused_f32_split_workspace(n, k, planes=3)), dtype=torch.uint8, device="cuda")
    Cs = torch.full_like(C, -5.0)
    assert gpu.spmma_fused_f32_split(dA, dB, Cs, m, n, k, ws, batch=batch, planes=3, check=False) == 0, "the split form must take every ResNet-18 layer"
    worst = ((Cs - C).abs() / Cd.clamp_min(1e-30)).max().item()
    assert worst <= SPLIT_TOL[3] + 4 * k * 2.0 ** -24, f"split (planes 3) vs exact: {worst:.3e} relative to sum|ab|"
    got = host(Cs[b * m * n: b * m * n + rows * n]).astype(np.float64)
    P64 = orc.decompress24(ob, rows, k, k, np.uint32).view(np.float32).astype(np.float64).reshape(rows, k)
    ref64 = (P64 @ Bh.astype(np.float64).reshape(k, n)).reshape(-1)
    bound = (SPLIT_TOL[3] + 2.0 * k * 2.0 ** -24) * scale + 2.0 ** -22 * np.abs(ref64) + 1e-30
    assert float((np.abs(got - ref64) / bound).max()) <= 1.0, "split (planes 3) sampled rows vs the oracle's operand in fp64"
    assert not (np.abs(got - Cref.astype(np.float64)) > FP32_TOL * np.maximum(scale, 1e-30)).any(), "split (planes 3) vs orc.spmma outside north_star's 1e-3"
    del C, Cd, P, blob, Cs, ws
    # the reference's own layout (gemm.hxx:80-81, examples/gemm.cu:60-90): column-major, pointer arrays, shared B
    Ccm = torch.full((batch * m * n,), -3.0, dtype=torch.float32, device="cuda")
    ptrs = lambda base, stride, cnt: torch.tensor([base.data_ptr() + 4 * stride * i for i in range(cnt)], dtype=torch.int64, device="cuda")
    gpu.gemm_batched(ptrs(dA, m * k, batch), ptrs(dB, 0, batch), ptrs(Ccm, m * n, batch), m, n, k, batch, "f32")
    ridx = np.unique(np.concatenate([np.arange(min(m, 8)), np.arange(max(m - 8, 0), m), np.random.default_rng(m).integers(0, m, 24)]))
    for bb in (0, batch - 1):
        Acm = host(dA[bb * m * k:(bb + 1) * m * k]).reshape(k, m)[:, ridx].T.astype(np.float64)   # column-major m x k, lda = m
        Bcm = Bh.reshape(n, k).T.astype(np.float64)                                          # column-major k x n, ldb = k
        want = Acm @ Bcm
        got = host(Ccm[bb * m * n:(bb + 1) * m * n]).reshape(n, m)[:, ridx].T
        check_close(got.reshape(-1), want.astype(np.float32).reshape(-1), (np.abs(Acm) @ np.abs(Bcm)).reshape(-1), FP32_TOL,
                    f"resnet18 f32 gemm_batched column-major sampled {shape} batch {bb}", k, "f32")


# ---------------------------------------------------------------------------------------------
# BASELINE.json config 5: unstructured 90 %-sparse COO x dense, fp32, on ResNet-50 shapes at b = 32
# (density 0.1, values U(-1,1): examples/batched_coo.cu:71, profiling/python/gemm_coo_compare.py:7,26)
# ---------------------------------------------------------------------------------------------
def _coo_problem(m, k, seed, density=0.1):
    rng = np.random.default_rng(seed)
    dense = rng.uniform(0, 1, (m, k)) < density
    r, c = np.nonzero(dense)                     # row-major scan: row-sorted, as the reference's driver emits it
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    return r.astype(np.int32), c.astype(np.int32), v, rng



def _coo_call(gpu, entry, m, k, nnz, n, batches, dr, dc, dv, dB, dC, alpha, beta, fill=0x5A):
    """sm_spmm_coo_f32_ws (row-pointer workspace) or sm_spmm_coo_f32_packed (padded, packed copy of A); the workspace is
    pre-filled with garbage: a stale one must not matter."""
    import ctypes
    import torch
    nb = ctypes.c_size_t(0)
    if entry == "ws":
        assert gpu.lib().sm_spmm_coo_workspace_size(m, ctypes.byref(nb)) == 0
        ws = torch.full((nb.value,), fill, dtype=torch.uint8, device="cuda")
        rc = gpu.lib().sm_spmm_coo_f32_ws(m, k, nnz, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(),
                                          dC.data_ptr(), alpha, beta, ws.data_ptr(), None)
    else:
        assert gpu.lib().sm_spmm_coo_packed_workspace_size(m, nnz, ctypes.byref(nb)) == 0
        ws = torch.full((nb.value,), fill, dtype=torch.uint8, device="cuda")
        rc = gpu.lib().sm_spmm_coo_f32_packed(m, k, nnz, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(),
                                               dC.data_ptr(), alpha, beta, ws.data_ptr(), nb.value, None)
    assert rc == 0, gpu.lib().sm_last_error()
    return ws


COO_FOUR = [(784, 256, 2304), (12544, 64, 576), (196, 512, 4608), (3136, 128, 1152)]
# every unique ResNet-50 shape (only four of the 17 were tested): the four above in both orders, the other 13 row-sorted
COO_CASES = [(s_, o) for s_ in COO_FOUR for o in ("sorted", "shuffled")] + [(s_, "sorted") for s_ in RESNET50_UNIQUE if s_ not in COO_FOUR]


@pytest.mark.parametrize("entry", ["ws", "packed"])
@pytest.mark.parametrize("shape,order", COO_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_spmm_coo_config5_resnet50_shapes(gpu, orc, shape, order, entry):
    """sm_spmm_coo_f32_ws at config 5's sizes: A m x k with ~10 % non-zeros shared by b = 32 batches, B_b k x n and
    C_b m x n column-major (spmm.hxx:164-187).  Row-sorted input takes the CSR kernels (the shapes pick J = 32 / 16 / 8
    vectors per workgroup and the row split), shuffled input the atomic fallback.  Sampled (row, column, batch) entries
    against the oracle run on the sub-problem made of exactly those rows and vectors."""
    import ctypes
    import torch
    m, n, k = shape
    batches = 32
    alpha, beta = 1.25, -0.5
    r, c, v, rng = _coo_problem(m, k, m + k)
    nnz = r.size
    if order == "shuffled":
        perm = rng.permutation(nnz)
        r, c, v = r[perm].copy(), c[perm].copy(), v[perm].copy()
    dB = torch.empty(batches * k * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dB, 0xC00 + n, -1.0, 1.0)
    dC = torch.empty(batches * m * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dC, 0xC0C + m, -1.0, 1.0)
    C0 = dC.clone()
    dr, dc, dv = to_dev(r), to_dev(c), to_dev(v)
    ws = _coo_call(gpu, entry, m, k, nnz, n, batches, dr, dc, dv, dB, dC, alpha, beta)
    if entry == "packed":   # the device-side decision: 4 = packed kernel (sorted rows), 1 = atomic fallback; k = 4608 is
        # beyond the packed form's LDS slab and runs as the row-pointer form (flag 0)
        assert int(host(ws[:4].view(torch.int32))[0]) == ((4 if k <= 2559 else 0) if order == "sorted" else 1)
    # sub-problem: sampled rows (first, last, random) x sampled vectors (batch, column)
    rs = np.unique(np.concatenate([[0, m - 1], rng.integers(0, m, 30)]))
    vecs = [(0, 0), (batches - 1, n - 1)] + [(int(rng.integers(0, batches)), int(rng.integers(0, n))) for _ in range(14)]
    remap = -np.ones(m, dtype=np.int64)
    remap[rs] = np.arange(rs.size)
    keep = remap[r] >= 0
    sr, sc, sv = remap[r[keep]].astype(np.int32), c[keep].copy(), v[keep].copy()
    Bh = np.concatenate([host(dB[(bb * n + j) * k:(bb * n + j + 1) * k]) for bb, j in vecs])       # [vec][k]: one "batch" with n = |vecs|
    C0h = host(C0).reshape(batches, n, m)
    Csub = np.stack([C0h[bb, j, rs] for bb, j in vecs]).astype(np.float32).reshape(-1)            # [vec][row]
    want = Csub.copy()
    orc.spmm_coo(rs.size, k, sr.size, len(vecs), 1, sr, sc, sv, Bh, want, alpha, beta)
    got = np.stack([host(dC).reshape(batches, n, m)[bb, j, rs] for bb, j in vecs]).reshape(-1)
    # scale = |alpha| sum |a| |b| + |beta| |c0| per sampled entry
    absA = np.zeros((rs.size, k))
    np.add.at(absA, (sr, sc), np.abs(sv.astype(np.float64)))
    scale = abs(alpha) * (np.abs(Bh.astype(np.float64)).reshape(len(vecs), k) @ absA.T).reshape(-1) + abs(beta) * np.abs(Csub)
    kmax = int(np.bincount(sr, minlength=rs.size).max())
    check_close(got, want, scale, FP32_TOL, f"config5 coo {shape} {order}", kmax + 2, "f32")
    # every output was produced (no stale C0 left where a row has non-zeros), spot check by the global checksum of
    # untouched-looking entries: rows without non-zeros must hold exactly beta * C0
    empty = np.setdiff1d(np.arange(m), np.unique(r))
    if empty.size:
        e = int(empty[0])
        assert np.array_equal(host(dC).reshape(batches, n, m)[:, :, e], (np.float32(beta) * C0h[:, :, e]).astype(np.float32))


def _coo_fast_call(gpu, m, k, nnz, n, batches, dr, dc, dv, dB, dC, alpha, beta):
    import ctypes
    import torch
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb)) == 0
    ws = torch.full((nb.value,), 0x5A, dtype=torch.uint8, device="cuda")   # stale workspace must not matter
    return gpu.lib().sm_spmm_coo_f32_fast(m, k, nnz, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(), dC.data_ptr(),
                                          alpha, beta, ws.data_ptr(), nb.value, None)


# bound of the dense-MFMA form: the dense operand rounded once to fp16 (2^-11 relative per element), A exact to 2^-22, fp32
# accumulation over k terms, one fp32 rounding of the result -- all relative to |alpha| sum|a||b| + |beta||c0|
COO_FAST_TOL = 2.0 ** -11 * 1.02


@pytest.mark.parametrize("shape,order", COO_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_spmm_coo_fast_config5_resnet50_shapes(gpu, orc, shape, order):
    """sm_spmm_coo_f32_fast (the fp16-split dense-MFMA form, an explicit opt-in) at config 5's sizes, b = 32: sampled entries
    against the fp64 oracle within COO_FAST_TOL of |alpha| sum|a||b| + |beta||c0| -- half of north_star's 1e-3 for fp32
    products, asserted exactly here -- for sorted and shuffled input (the scatter does not care), alpha / beta != (1, 0)."""
    import torch
    m, n, k = shape
    batches = 32
    alpha, beta = 1.25, -0.5
    r, c, v, rng = _coo_problem(m, k, m + k)
    nnz = r.size
    if order == "shuffled":
        perm = rng.permutation(nnz)
        r, c, v = r[perm].copy(), c[perm].copy(), v[perm].copy()
    dB = torch.empty(batches * k * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dB, 0xC00 + n, -1.0, 1.0)
    dC = torch.empty(batches * m * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dC, 0xC0C + m, -1.0, 1.0)
    C0 = dC.clone()
    dr, dc, dv = to_dev(r), to_dev(c), to_dev(v)
    rc = _coo_fast_call(gpu, m, k, nnz, n, batches, dr, dc, dv, dB, dC, alpha, beta)
    if k % 64 != 0:   # the stem layer's k = 147: the dense-MFMA form declines (whole 64-deep stages only) and says so
        assert rc == gpu.STATUS_NOT_SUPPORTED and torch.equal(dC, C0)
        return
    assert rc == 0, gpu.lib().sm_last_error()
    rs = np.unique(np.concatenate([[0, m - 1], rng.integers(0, m, 30)]))
    vecs = [(0, 0), (batches - 1, n - 1)] + [(int(rng.integers(0, batches)), int(rng.integers(0, n))) for _ in range(14)]
    remap = -np.ones(m, dtype=np.int64)
    remap[rs] = np.arange(rs.size)
    keep = remap[r] >= 0
    sr, sc, sv = remap[r[keep]].astype(np.int32), c[keep].copy(), v[keep].copy()
    Bh = np.concatenate([host(dB[(bb * n + j) * k:(bb * n + j + 1) * k]) for bb, j in vecs])
    C0h = host(C0).reshape(batches, n, m)
    Csub = np.stack([C0h[bb, j, rs] for bb, j in vecs]).astype(np.float32).reshape(-1)
    want = Csub.copy()
    orc.spmm_coo(rs.size, k, sr.size, len(vecs), 1, sr, sc, sv, Bh, want, alpha, beta)
    got = np.stack([host(dC).reshape(batches, n, m)[bb, j, rs] for bb, j in vecs]).reshape(-1)
    absA = np.zeros((rs.size, k))
    np.add.at(absA, (sr, sc), np.abs(sv.astype(np.float64)))
    scale = abs(alpha) * (np.abs(Bh.astype(np.float64)).reshape(len(vecs), k) @ absA.T).reshape(-1) + abs(beta) * np.abs(Csub)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float(np.max(err / np.maximum(scale, 1e-30)))
    assert worst <= COO_FAST_TOL, f"fast coo {shape} {order}: worst error {worst:.3e} of the scale, bound {COO_FAST_TOL:.3e}"
    assert worst <= 1e-3   # north_star's fp32 tolerance
    empty = np.setdiff1d(np.arange(m), np.unique(r))
    if empty.size:   # rows without non-zeros: beta * C0 (+ 0), exactly
        e = int(empty[0])
        assert np.array_equal(host(dC).reshape(batches, n, m)[:, :, e], (np.float32(beta) * C0h[:, :, e]).astype(np.float32))


@pytest.mark.parametrize("shape", [(8, 8, 64, 1), (132, 33, 128, 3), (300, 130, 256, 2), (20, 5, 192, 4), (128, 64, 64, 2)], ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("order", ["sorted", "shuffled", "duplicates"])
def test_spmm_coo_fast_small_vs_oracle(gpu, orc, shape, order):
    """Every output of the dense-MFMA form on small shapes (ragged tiles, duplicates, an empty matrix, beta = 0) within its
    bound; shapes it does not take (cols % 64, rows % 4, a short workspace) return SM_STATUS_NOT_SUPPORTED untouched."""
    import ctypes
    import torch
    m, n, k, batches = shape
    rng = np.random.default_rng(m * 7 + n + k)
    dens = rng.uniform(0, 1, (m, k)) < 0.15
    r, c = np.nonzero(dens)
    r, c = r.astype(np.int32), c.astype(np.int32)
    if order == "duplicates" and r.size:
        r, c = np.concatenate([r, r[:50]]), np.concatenate([c, c[:50]])
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    if order == "shuffled":
        p_ = rng.permutation(r.size)
        r, c, v = r[p_].copy(), c[p_].copy(), v[p_].copy()
    B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
    for alpha, beta in ((1.0, 0.0), (0.75, 2.0)):
        C0 = rng.uniform(-1, 1, batches * m * n).astype(np.float32)
        dC = to_dev(C0.copy())
        rc = _coo_fast_call(gpu, m, k, r.size, n, batches, to_dev(r) if r.size else torch.zeros(1, dtype=torch.int32, device="cuda"),
                            to_dev(c) if r.size else torch.zeros(1, dtype=torch.int32, device="cuda"),
                            to_dev(v) if r.size else torch.zeros(1, dtype=torch.float32, device="cuda"), to_dev(B), dC, alpha, beta)
        assert rc == 0, gpu.lib().sm_last_error()
        want = C0.copy()
        orc.spmm_coo(m, k, r.size, n, batches, r, c, v, B, want, alpha, beta)
        absA = np.zeros((m, k))
        np.add.at(absA, (r, c), np.abs(v.astype(np.float64)))
        scale = np.concatenate([(abs(alpha) * (np.abs(B[bb * k * n:(bb + 1) * k * n].astype(np.float64)).reshape(n, k) @ absA.T)).reshape(-1) for bb in range(batches)])
        scale = scale + abs(beta) * np.abs(C0)
        err = np.abs(host(dC).astype(np.float64) - want.astype(np.float64))
        assert float(np.max(err / np.maximum(scale, 1e-30))) <= COO_FAST_TOL
    # declined shapes leave C alone
    L = gpu.lib()
    nb = ctypes.c_size_t(0)
    L.sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb))
    ws = torch.zeros(max(nb.value, 16), dtype=torch.uint8, device="cuda")
    dC = to_dev(C0.copy())
    z = lambda t: t.data_ptr()
    dr, dc_, dv = (to_dev(r), to_dev(c), to_dev(v)) if r.size else (torch.zeros(1, dtype=torch.int32, device="cuda"),) * 2 + (torch.zeros(1, dtype=torch.float32, device="cuda"),)
    dB = to_dev(B)
    assert L.sm_spmm_coo_f32_fast(m, k + 1, r.size, n, batches, z(dr), z(dc_), z(dv), z(dB), z(dC), 1.0, 0.0, z(ws), nb.value, None) == 2   # cols % 64
    assert L.sm_spmm_coo_f32_fast(m, k, r.size, n, batches, z(dr), z(dc_), z(dv), z(dB), z(dC), 1.0, 0.0, z(ws), max(nb.value, 16) - 16, None) == 2   # short workspace
    assert np.array_equal(host(dC), C0)


@pytest.mark.parametrize("mag_b,mag_a", [(1e-6, 1.0), (3e5, 1.0), (1e-20, 1e-12), (1e12, 1e10), (1.0, 1e-30)], ids=lambda v: "%g" % v)
def test_spmm_coo_fast_holds_its_bound_at_any_magnitude(gpu, orc, mag_b, mag_a):
    """the fp16-split form cast its operands straight to fp16 -- uniformly small operands (activations
    ~1e-6) fell below fp16's normal range and came back with percent-level error while the call returned SUCCESS, large ones
    overflowed.  Round 4: power-of-two scales computed on the device (largest |b| of a strided sample -> [2^12, 2^13), largest |a|
    -> [2^13, 2^14)) and folded back into the fp32 sums, so the 2^-11 bound holds whatever the magnitude, and the range flag stays 0."""
    import ctypes
    import torch
    m, n, k, batches = 260, 72, 192, 3
    rng = np.random.default_rng(77)
    dens = rng.uniform(0, 1, (m, k)) < 0.1
    r, c = np.nonzero(dens)
    r, c = r.astype(np.int32), c.astype(np.int32)
    v = (rng.uniform(-1, 1, r.size) * mag_a).astype(np.float32)
    B = (rng.uniform(-1, 1, batches * k * n) * mag_b).astype(np.float32)
    C0 = np.zeros(batches * m * n, dtype=np.float32)
    dC = to_dev(C0.copy())
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb)) == 0
    ws = torch.full((nb.value,), 0x5A, dtype=torch.uint8, device="cuda")
    dr, dc_, dv, dB = to_dev(r), to_dev(c), to_dev(v), to_dev(B)
    rc = gpu.lib().sm_spmm_coo_f32_fast(m, k, r.size, n, batches, dr.data_ptr(), dc_.data_ptr(), dv.data_ptr(), dB.data_ptr(), dC.data_ptr(),
                                        1.0, 0.0, ws.data_ptr(), nb.value, None)
    assert rc == 0, gpu.lib().sm_last_error()
    flag = ctypes.c_int(-1)
    assert gpu.lib().sm_spmm_coo_fast_flag(ws.data_ptr(), ctypes.byref(flag), None) == 0 and flag.value == 0
    want = np.zeros(batches * m * n, dtype=np.float64)
    A64 = np.zeros((m, k))
    np.add.at(A64, (r, c), v.astype(np.float64))
    absA = np.abs(A64)
    for bb in range(batches):
        Bb = B[bb * k * n:(bb + 1) * k * n].astype(np.float64).reshape(n, k)
        want[bb * m * n:(bb + 1) * m * n] = (Bb @ A64.T).reshape(-1)
    scale = np.concatenate([(np.abs(B[bb * k * n:(bb + 1) * k * n].astype(np.float64)).reshape(n, k) @ absA.T).reshape(-1) for bb in range(batches)])
    err = np.abs(host(dC).astype(np.float64) - want)
    # + the absolute term of the stated bound: 2^-37 max|b| sum|a| (elements far below the largest one)
    extra = 2.0 ** -37 * float(np.abs(B).max()) * np.tile(absA.sum(axis=1), batches * n).reshape(batches, n, m).reshape(-1)
    worst = float(np.max(err / np.maximum(COO_FAST_TOL * scale + extra, 1e-300)))
    assert worst <= 1.0, f"scaled fast coo at |b| ~ {mag_b:g}, |a| ~ {mag_a:g}: worst error / bound = {worst:.3f}"


def test_spmm_coo_fast_flags_what_does_not_convert_and_leaves_c_alone(gpu):
    """An element the scales cannot bring into the fp16 range (inf, NaN, or far above the sampled maximum) raises the flag on the
    device and the matrix kernel returns without writing C: the caller (sparsifyme::batched::strided_coo) then runs the exact form
    on untouched operands."""
    import ctypes
    import torch
    m, n, k, batches = 128, 64, 64, 2
    rng = np.random.default_rng(5)
    r = np.repeat(np.arange(m, dtype=np.int32), 4)
    c = rng.integers(0, k, r.size).astype(np.int32)
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    nb = ctypes.c_size_t(0)
    gpu.lib().sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb))
    for poison in (np.float32("inf"), np.float32("nan")):
        B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
        B[777] = poison
        C0 = rng.uniform(-1, 1, batches * m * n).astype(np.float32)
        dC = to_dev(C0.copy())
        ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        dr, dc_, dv, dB = to_dev(r), to_dev(c), to_dev(v), to_dev(B)
        rc = gpu.lib().sm_spmm_coo_f32_fast(m, k, r.size, n, batches, dr.data_ptr(), dc_.data_ptr(), dv.data_ptr(), dB.data_ptr(), dC.data_ptr(),
                                            1.0, 0.5, ws.data_ptr(), nb.value, None)
        assert rc == 0
        flag = ctypes.c_int(0)
        assert gpu.lib().sm_spmm_coo_fast_flag(ws.data_ptr(), ctypes.byref(flag), None) == 0 and flag.value != 0
        assert np.array_equal(host(dC), C0), "C was written although the range flag is up"
    # k == 0 and overflowing sizes are declined, not mis-sized
    huge = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_fast_workspace_size(1 << 40, 1 << 40, 1 << 20, 1 << 20, ctypes.byref(huge)) == gpu.STATUS_NOT_SUPPORTED
    dC = to_dev(np.ones(8 * 8, dtype=np.float32))
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert gpu.lib().sm_spmm_coo_f32_fast(8, 0, 0, 8, 1, None, None, None, z.data_ptr(), dC.data_ptr(), 1.0, 0.0, z.data_ptr(), 64, None) == gpu.STATUS_NOT_SUPPORTED


def _coo_fast_check(gpu, orc, m, n, k, batches, r, c, v, B, alpha, tol=None):
    """one beta == 0 call of sm_spmm_coo_f32_fast against the oracle on every output; returns (flag, C)"""
    import ctypes
    import torch
    C0 = np.full(batches * m * n, 7.0, dtype=np.float32)
    dC = to_dev(C0.copy())
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb)) == 0
    ws = torch.full((nb.value,), 0x5A, dtype=torch.uint8, device="cuda")
    one = lambda dt: torch.zeros(1, dtype=dt, device="cuda")
    dr, dc_, dv = (to_dev(r), to_dev(c), to_dev(v)) if r.size else (one(torch.int32), one(torch.int32), one(torch.float32))
    dB = to_dev(B)
    rc = gpu.lib().sm_spmm_coo_f32_fast(m, k, r.size, n, batches, dr.data_ptr(), dc_.data_ptr(), dv.data_ptr(), dB.data_ptr(), dC.data_ptr(), alpha, 0.0,
                                        ws.data_ptr(), nb.value, None)
    assert rc == 0, gpu.lib().sm_last_error()
    flag = ctypes.c_int(-1)
    assert gpu.lib().sm_spmm_coo_fast_flag(ws.data_ptr(), ctypes.byref(flag), None) == 0
    got = host(dC)
    if flag.value == 0:
        want = C0.copy()
        orc.spmm_coo(m, k, r.size, n, batches, r, c, v, B, want, alpha, 0.0)
        absA = np.zeros((m, k))
        np.add.at(absA, (r, c), np.abs(v.astype(np.float64)))
        scale = np.concatenate([(abs(alpha) * (np.abs(B[bb * k * n:(bb + 1) * k * n].astype(np.float64)).reshape(n, k) @ absA.T)).reshape(-1) for bb in range(batches)])
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        worst = float(np.max(err / np.maximum(scale, 1e-30)))
        assert worst <= (tol or COO_FAST_TOL), f"sparse-instruction coo {m}x{n}x{k}x{batches}: worst error {worst:.3e} of the scale"
        assert np.array_equal(got[scale == 0], np.zeros(int((scale == 0).sum()), dtype=np.float32))   # nothing to add: exactly alpha * 0
    return flag.value, got


@pytest.mark.parametrize("shape", [(8, 8, 64, 1), (132, 33, 128, 3), (300, 130, 250, 2), (20, 5, 192, 4), (128, 64, 64, 2), (260, 72, 147, 3), (64, 40, 90, 2),
                                   (516, 24, 200, 5), (4, 3, 7, 1), (1000, 16, 1148, 2), (256, 200, 512, 1), (196, 130, 1152, 2), (68, 40, 200, 3), (200, 16, 448, 1)], ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("order", ["sorted", "shuffled", "duplicates", "dense_strips"])
def test_spmm_coo_smfmac_small_vs_oracle(gpu, orc, shape, order):
    """The sparse-matrix-instruction form of sm_spmm_coo_f32_fast (beta == 0, density <= 20 %: sm_spmm_coo_fast_form == 2) on every output
    against the oracle, inside the dense-MFMA form's bound: ragged row / column tiles, k % 64 != 0 and k % 4 != 0 (the stem layer's 147),
    unsorted input, duplicates (added), strips with three and four non-zeros (the bucket entries), an empty matrix."""
    m, n, k, batches = shape
    rng = np.random.default_rng(m * 7 + n + k)
    dens = rng.uniform(0, 1, (m, k)) < (0.07 if order == "dense_strips" else 0.15)
    if order == "dense_strips":   # whole strips and runs of three on top of a sparse background; still under 20 %
        for _ in range(max(1, m * k // 80)):
            i, j = int(rng.integers(0, m)), int(rng.integers(0, max(1, k - 4)))
            dens[i, j:j + int(rng.integers(3, 6))] = True
    r, c = np.nonzero(dens)
    r, c = r.astype(np.int32), c.astype(np.int32)
    if order == "duplicates" and r.size:
        r, c = np.concatenate([r, r[:50]]), np.concatenate([c, c[:50]])
    r, c = r[:m * k // 5], c[:m * k // 5]     # (tiny shapes: stay under the 20 % the form takes)
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    if order == "shuffled":
        p_ = rng.permutation(r.size)
        r, c, v = r[p_].copy(), c[p_].copy(), v[p_].copy()
    B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
    assert r.size * 5 <= m * k and gpu.lib().sm_spmm_coo_fast_form(m, k, r.size, n, batches, 0.0) == 2
    assert gpu.lib().sm_spmm_coo_fast_form(m, k, r.size, n, batches, 0.5) == (1 if k % 64 == 0 and m >= 8 else 0)
    flag, _ = _coo_fast_check(gpu, orc, m, n, k, batches, r, c, v, B, 0.75)
    assert flag == 0
    if order == "sorted":   # an empty matrix: C = 0 exactly
        e = np.zeros(0, dtype=np.int32)
        flag, got = _coo_fast_check(gpu, orc, m, n, k, batches, e, e, np.zeros(0, dtype=np.float32), B, 1.0)
        assert flag == 0 and not got.any()


def test_spmm_coo_smfmac_is_reproducible_and_exact_on_integers(gpu):
    """Small-integer data (every product and sum exact in fp16 x fp32): the sparse-instruction form equals the integer product bit for bit --
    image, index nibbles, bucket entries and the result map all in place -- and two calls give the same bits."""
    import ctypes
    import torch
    m, n, k, batches = 388, 150, 328, 2
    rng = np.random.default_rng(99)
    dens = rng.uniform(0, 1, (m, k)) < 0.17
    r, c = np.nonzero(dens)
    r, c = r.astype(np.int32), c.astype(np.int32)
    v = rng.integers(-8, 9, r.size).astype(np.float32)
    B = rng.integers(-8, 9, batches * k * n).astype(np.float32)
    A = np.zeros((m, k))
    np.add.at(A, (r, c), v.astype(np.float64))
    want = np.concatenate([(B[bb * k * n:(bb + 1) * k * n].astype(np.float64).reshape(n, k) @ A.T).reshape(-1) for bb in range(batches)]) * 2.0
    nb = ctypes.c_size_t(0)
    gpu.lib().sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb))
    outs = []
    for _ in range(2):
        ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        dC = torch.full((batches * m * n,), 3.0, device="cuda")
        dr, dc_, dv, dB = to_dev(r), to_dev(c), to_dev(v), to_dev(B)
        assert gpu.lib().sm_spmm_coo_f32_fast(m, k, r.size, n, batches, dr.data_ptr(), dc_.data_ptr(), dv.data_ptr(), dB.data_ptr(), dC.data_ptr(), 2.0, 0.0,
                                              ws.data_ptr(), nb.value, None) == 0
        outs.append(host(dC))
    assert np.array_equal(outs[0].astype(np.float64), want) and np.array_equal(outs[0], outs[1])


def test_spmm_coo_smfmac_flags(gpu, orc):
    """The sparse-instruction form's flag: a non-finite or far-out-of-range element of B -> flag, the tiles that read it left alone (here: one
    tile = all of C); a non-finite A value or a 128 x 64 block with more third / fourth non-zeros than its bucket holds -> flag, C untouched;
    and the same operands under 2^30 and 2^-30 convert (the scales), flag 0."""
    m, n, k, batches = 128, 32, 64, 2
    rng = np.random.default_rng(5)
    r = np.repeat(np.arange(m, dtype=np.int32), 4)
    c = rng.integers(0, k, r.size).astype(np.int32)
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
    for poison in (np.float32("inf"), np.float32("nan")):
        Bp = B.copy()
        Bp[777] = poison
        flag, got = _coo_fast_check(gpu, orc, m, n, k, batches, r, c, v, Bp, 1.0)
        assert flag != 0 and np.array_equal(got, np.full(got.size, 7.0, dtype=np.float32))
    vp = v.copy()
    vp[100] = np.float32("inf")
    flag, got = _coo_fast_check(gpu, orc, m, n, k, batches, r, c, vp, B, 1.0)
    assert flag != 0 and np.array_equal(got, np.full(got.size, 7.0, dtype=np.float32))
    for mag in (2.0 ** 30, 2.0 ** -30):
        flag, _ = _coo_fast_check(gpu, orc, m, n, k, batches, r, c, (v * mag).astype(np.float32), (B * mag).astype(np.float32), 1.0)
        assert flag == 0
    # one fully dense 128 x 64 block inside a 1024 x 64 matrix (12.5 % dense overall): 4096 third / fourth non-zeros in one bucket of 256
    m2 = 1024
    rr, cc = np.meshgrid(np.arange(128, dtype=np.int32), np.arange(64, dtype=np.int32), indexing="ij")
    r2, c2 = rr.reshape(-1).copy(), cc.reshape(-1).copy()
    v2 = rng.uniform(-1, 1, r2.size).astype(np.float32)
    assert gpu.lib().sm_spmm_coo_fast_form(m2, k, r2.size, n, batches, 0.0) == 2
    flag, got = _coo_fast_check(gpu, orc, m2, n, k, batches, r2, c2, v2, B, 1.0)
    assert flag != 0 and np.array_equal(got, np.full(got.size, 7.0, dtype=np.float32))
    # the same block at a quarter of the rows' strips full (two per strip: nothing for the buckets) is fine
    keep = (c2 % 4) < 2
    flag, _ = _coo_fast_check(gpu, orc, m2, n, k, batches, r2[keep], c2[keep], v2[keep], B, 1.0)
    assert flag == 0


@pytest.mark.parametrize("shape", [s_ for s_, o_ in COO_CASES if o_ == "sorted"], ids=lambda v: "x".join(map(str, v)))
def test_spmm_coo_smfmac_config5_resnet50_shapes(gpu, orc, shape):
    """sm_spmm_coo_f32_fast with beta == 0 at config 5's sizes (b = 32, 10 % dense, every ResNet-50 shape incl. k = 147): the sparse-instruction
    form (k <= 128, matrices of at most 256 rows, ragged k) or the dense-MFMA pipeline (sm_spmm_coo_fast_form says which): sampled rows x vectors
    against the fp64 oracle within the bound."""
    import ctypes
    import torch
    m, n, k = shape
    batches = 32
    alpha = 1.25
    r, c, v, rng = _coo_problem(m, k, m + k)
    nnz = r.size
    form = gpu.lib().sm_spmm_coo_fast_form(m, k, nnz, n, batches, 0.0)
    # the rule of coo_smfmac_takes: where the dense-MFMA pipeline applies (k % 64 == 0) it keeps the longer-K shapes
    nst = -(-k // 64)
    assert form == (2 if k % 64 != 0 or nst <= 2 or m <= 256 else 1)
    dB = torch.empty(batches * k * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dB, 0xC00 + n, -1.0, 1.0)
    dC = torch.full((batches * m * n,), 5.0, dtype=torch.float32, device="cuda")
    dr, dc, dv = to_dev(r), to_dev(c), to_dev(v)
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_fast_workspace_size(m, k, n, batches, ctypes.byref(nb)) == 0
    ws = torch.full((nb.value,), 0x5A, dtype=torch.uint8, device="cuda")
    assert gpu.lib().sm_spmm_coo_f32_fast(m, k, nnz, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(), dC.data_ptr(), alpha, 0.0,
                                          ws.data_ptr(), nb.value, None) == 0, gpu.lib().sm_last_error()
    flag = ctypes.c_int(-1)
    assert gpu.lib().sm_spmm_coo_fast_flag(ws.data_ptr(), ctypes.byref(flag), None) == 0 and flag.value == 0
    rs = np.unique(np.concatenate([[0, m - 1, 127, 128], rng.integers(0, m, 40)]))
    rs = rs[rs < m]
    vecs = [(0, 0), (batches - 1, n - 1)] + [(int(rng.integers(0, batches)), int(rng.integers(0, n))) for _ in range(14)]
    remap = -np.ones(m, dtype=np.int64)
    remap[rs] = np.arange(rs.size)
    keep = remap[r] >= 0
    sr, sc, sv = remap[r[keep]].astype(np.int32), c[keep].copy(), v[keep].copy()
    Bh = np.concatenate([host(dB[(bb * n + j) * k:(bb * n + j + 1) * k]) for bb, j in vecs])
    want = np.zeros(len(vecs) * rs.size, dtype=np.float32)
    orc.spmm_coo(rs.size, k, sr.size, len(vecs), 1, sr, sc, sv, Bh, want, alpha, 0.0)
    Ch = host(dC).reshape(batches, n, m)
    got = np.stack([Ch[bb, j, rs] for bb, j in vecs]).reshape(-1)
    absA = np.zeros((rs.size, k))
    np.add.at(absA, (sr, sc), np.abs(sv.astype(np.float64)))
    scale = abs(alpha) * (np.abs(Bh.astype(np.float64)).reshape(len(vecs), k) @ absA.T).reshape(-1)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float(np.max(err / np.maximum(scale, 1e-30)))
    assert worst <= COO_FAST_TOL, f"sparse-instruction coo {shape}: worst error {worst:.3e} of the scale, bound {COO_FAST_TOL:.3e}"
    empty = np.setdiff1d(np.arange(m), np.unique(r))
    if empty.size:   # rows without non-zeros: exactly zero
        assert not Ch[:, :, int(empty[0])].any()
    assert np.isfinite(Ch).all()


@pytest.mark.parametrize("shape", [(150, 33, 90, 3), (64, 9, 48, 2), (300, 130, 260, 1), (17, 5, 129, 4), (129, 64, 128, 2), (50, 70, 1000, 3), (33, 300, 52, 1)],
                         ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("order", ["sorted", "cols_shuffled_within_rows", "shuffled", "duplicates"])
@pytest.mark.parametrize("entry", ["ws", "packed"])
def test_spmm_coo_ws_orders_vs_oracle(gpu, orc, shape, order, entry):
    """sm_spmm_coo_f32_ws on small shapes against the oracle on every entry: row-sorted input (columns sorted or not,
    duplicates included) takes the CSR kernel, fully shuffled input the atomic kernels; all four must agree."""
    import ctypes
    import torch
    m, n, k, batches = shape
    r, c, v, rng = _coo_problem(m, k, m * 7 + k, 0.15)
    if order == "duplicates":
        r, c = np.concatenate([r, r[::7]]), np.concatenate([c, c[::7]])
        v = np.concatenate([v, rng.uniform(-1, 1, r.size - v.size).astype(np.float32)])
        o = np.lexsort((c, r))
        r, c, v = r[o].copy(), c[o].copy(), v[o].copy()
    elif order == "cols_shuffled_within_rows":
        o = np.lexsort((rng.permutation(r.size), r))
        r, c, v = r[o].copy(), c[o].copy(), v[o].copy()
    elif order == "shuffled":
        o = rng.permutation(r.size)
        r, c, v = r[o].copy(), c[o].copy(), v[o].copy()
    B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
    C0 = rng.uniform(-1, 1, batches * m * n).astype(np.float32)
    want = C0.copy()
    orc.spmm_coo(m, k, r.size, n, batches, r, c, v, B, want, 1.5, -0.75)
    dC, dr, dc, dv, dB = to_dev(C0.copy()), to_dev(r), to_dev(c), to_dev(v), to_dev(B)
    _coo_call(gpu, entry, m, k, r.size, n, batches, dr, dc, dv, dB, dC, 1.5, -0.75, fill=0xA5)
    assert np.allclose(host(dC), want, rtol=2e-5, atol=2e-5), f"max diff {np.abs(host(dC) - want).max():.3e}"


@pytest.mark.parametrize("entry", ["ws", "packed"])
def test_spmm_coo_rejects_nothing_but_routes_bad_rows_to_the_atomic_kernel(gpu, orc, entry):
    """Row indices outside [0, rows) (the cuSPARSE call would be undefined) are skipped entry by entry, never used as
    CSR row pointers: a negative index in an otherwise sorted list must not displace valid entries."""
    import ctypes
    import torch
    m, k, n, batches = 64, 48, 9, 2
    r, c, v, rng = _coo_problem(m, k, 77, 0.2)
    r2 = r.copy()
    r2[0] = -3
    r2[-1] = m + 5
    B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
    want = np.zeros(batches * m * n, dtype=np.float32)
    ok = (r2 >= 0) & (r2 < m)
    orc.spmm_coo(m, k, int(ok.sum()), n, batches, r2[ok].copy(), c[ok].copy(), v[ok].copy(), B, want, 1.0, 0.0)
    dC = torch.full((batches * m * n,), 5.0, dtype=torch.float32, device="cuda")
    dr, dc, dv, dB = to_dev(r2), to_dev(c), to_dev(v), to_dev(B)
    _coo_call(gpu, entry, m, k, r2.size, n, batches, dr, dc, dv, dB, dC, 1.0, 0.0, fill=0)
    assert np.allclose(host(dC), want, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# the drop-in boundary end to end: the C++ drivers (header-only API -> C ABI -> HIP kernels)
# ---------------------------------------------------------------------------------------------
def test_cpp_drivers_cli_contract(gpu):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bins = os.path.join(root, "examples", "bin")
    if not os.path.exists(os.path.join(bins, "spmma_i8")):
        subprocess.run(["make", "-C", os.path.join(root, "examples"), "-j4"], check=True, capture_output=True)

    def run(*args):
        return subprocess.run([os.path.join(bins, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=120)
    for tool, argv in [("sparsify", (512, 512)), ("gemm", (196, 64, 128, 4)), ("spmm", (64, 32, 64, 2)), ("batched_coo", (64, 16, 48, 2))]:
        out = run(tool, *argv)
        assert out.returncode == 0, out.stderr
        assert float(out.stdout.strip()) > 0.0
    out = run("spmma", 196, 64, 128, 4)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and [l.split(":")[0] for l in lines] == ["Pruning Time (ms)", "Compression Time (ms)", "SpMMA Time (ms)"]
    assert "Incorrect pruning" not in out.stderr
    # default (round 6): THREE measured, non-zero stage times on every shape, as the reference returns and prints them (spmma.hxx:117,
    # examples/spmma.cu:64-66): one-pass prune + check + compress | blob allocation | multiply
    vals = [float(l.split(":")[1]) for l in lines]
    assert all(v > 0.0 for v in vals)
    out = run("spmma", 196, 256, 128, 4)
    vals = [float(l.split(":")[1]) for l in out.stdout.strip().splitlines()]
    assert out.returncode == 0 and all(v > 0.0 for v in vals) and "Incorrect pruning" not in out.stderr
    # opt-in (spmma_options().fewest_passes; the driver's optional fifth argument): the whole sequence through sm_prune24_spmma_f16, no
    # blob -- one measured time, reported first; nothing compressed, no separately timed multiply
    for shape_ in [(196, 64, 128, 4), (196, 256, 128, 4)]:
        out = run("spmma", *shape_, "fewest")
        vals = [float(l.split(":")[1]) for l in out.stdout.strip().splitlines()]
        assert out.returncode == 0 and vals[0] > 0.0 and vals[1] == 0.0 and vals[2] == 0.0 and "Incorrect pruning" not in out.stderr
    assert run("spmma", 196, 64, 128, 4, "nonsense").returncode != 0
    # the reference's own instantiation (type_t = float, examples/spmma.cu:24): one-pass prune + check + compress since round 3
    if not os.path.exists(os.path.join(bins, "spmma_f32")):
        subprocess.run(["make", "-C", os.path.join(root, "examples"), "-j4"], check=True, capture_output=True)
    out = run("spmma_f32", 196, 64, 128, 4)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and [l.split(":")[0] for l in lines] == ["Pruning Time (ms)", "Compression Time (ms)", "SpMMA Time (ms)"]
    assert all(float(l.split(":")[1]) > 0.0 for l in lines) and "Incorrect pruning" not in out.stderr
    # ... and with the multiply on the sparse matrix instruction (spmma_options().f32_planes = 3): same three labels
    out = run("spmma_f32", 196, 64, 128, 4, 3)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and [l.split(":")[0] for l in lines] == ["Pruning Time (ms)", "Compression Time (ms)", "SpMMA Time (ms)"]
    assert float(lines[0].split(":")[1]) > 0.0 and float(lines[2].split(":")[1]) > 0.0 and "Incorrect pruning" not in out.stderr
    assert run("spmma_f32", 196, 64, 128, 4, 5).returncode != 0
    bad = run("spmma", 1, 2)
    assert bad.returncode != 0 and "Usage: ./spmma m n k b" in bad.stdout
    # int8 driver: stage labels of the fp16 one; its fused kernel must return the staged pair's bytes
    for argv in [(196, 64, 128, 4), (784, 256, 1152, 2), (130, 72, 192, 3)]:
        out = run("spmma_i8", *argv)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "SpMMA Time (ms)" in out.stdout and "Fused matches: yes" in out.stdout
    # transposed operands of spmma() (reference spmma.hxx:30-31,67-69) through the header: C and the in-place pruned
    # A of the four (transpose_a, transpose_b) pairs must be those of the (N, N) call on the N-form data
    for argv in [(196, 64, 128, 2), (130, 72, 200, 3), (64, 64, 64, 1)]:
        out = run("spmma_ops", *argv)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.count("matches N,N: yes") == 4 and "Incorrect pruning" not in out.stderr
    # the sweep harness (row a7; reference examples/profiling.py:4-44): the reference's seven columns first, one row per layer
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        tab, res = os.path.join(td, "three.csv"), os.path.join(td, "compare.csv")
        with open(tab, "w") as fh:
            fh.write("m,n,k,b\n784,64,128,4\n196,128,256,2\n392,72,64,3\n")
        out = subprocess.run([os.path.join(bins, "sweep"), tab, res], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Incorrect pruning" not in out.stderr
        rows = [l.strip().split(",") for l in open(res)]
        assert rows[0][:7] == ["m", "n", "k", "b", "gemm", "prune", "spmm"]
        assert rows[0][7:10] == ["spmma_prune", "spmma_compress", "spmma_mul"]
        assert len(rows) == 4 and [r[:4] for r in rows[1:]] == [["784", "64", "128", "4"], ["196", "128", "256", "2"], ["392", "72", "64", "3"]]
        assert all(float(x) > 0.0 for r in rows[1:] for x in r[4:10])
        # round 4: one spmma() call as callers get it (the one-kernel form on these shapes) beside the three staged stages
        assert rows[0][12] == "spmma_call" and all(0.0 < float(r[12]) for r in rows[1:])
    # cached-plan form (row f-1): compress once, multiply many; the driver compares its C with spmma()'s bit for bit
    for argv in [(196, 64, 128, 4), (784, 256, 1152, 2), (130, 72, 200, 3)]:
        for tool in ("spmma_plan", "spmma_plan_bf16"):
            out = run(tool, *argv, 3)
            assert out.returncode == 0, out.stdout + out.stderr
            assert "Matches spmma(): yes" in out.stdout


def test_values_through_the_cpp_headers_vs_oracle(gpu):
    """Row b of the scope table, by VALUE: tests/cpp/header_parity runs sparsify<2,2>, batched::gemm (N,N and T,N),
    batched::spmm, batched::strided_coo, spmma<half / float> (N,N and T,N; float also with spmma_options().f32_planes = 3 / 2) and spmma_f32_planes_t (prepared planes == spmma_fused<float>, bit for bit) through include/sparsify.me/*.hxx on a 3-row
    table and compares every result with the oracle (bit-exact masks / pruned A, the tight GEMM bound for the products).
    `--swap` then rotates the C pointer table handed to batched::gemm / batched::spmm: every such check must notice, i.e. a
    swapped pointer inside a header would turn this test red."""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "bin", "header_parity")
    subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp")], check=True, capture_output=True)
    with tempfile.TemporaryDirectory() as td:
        tab = os.path.join(td, "three.csv")
        with open(tab, "w") as fh:
            fh.write("m,n,k,b\n196,64,128,3\n64,40,72,2\n130,24,64,4\n")
        out = subprocess.run([exe, tab], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
        assert "MISMATCH" not in out.stdout and "Incorrect pruning" not in out.stderr
        assert out.stdout.count(" ok") >= 3 * (3 + 1 + 1 + 1 + 4 + 4 + 12) + 2 + 4   # (T,N) gemm only where m >= k (the reference's lda = m); spmma<float> also with f32_planes = 3 / 2; spmma_f32_planes_t on the two k % 64 == 0 rows
        assert out.stdout.count("spmma_f32_planes_t") == 4
        sw = subprocess.run([exe, tab, "--swap"], capture_output=True, text=True, timeout=600)
        assert sw.returncode == 0, sw.stdout[-4000:] + sw.stderr[-2000:]
        assert sw.stdout.count("rotated pointer table detected") >= 3 * 2 + 2 and "did not notice" not in sw.stdout


def test_sparsify_namespace_alias_through_the_headers(gpu):
    """The `sparsify::` spelling BASELINE's north_star uses (sparsify::sparsify / spmma / spmm / gemm): opt-in through
    -DSPARSIFYME_NAMESPACE_ALIAS (include/sparsify.me/util/alias.hxx; SURVEY.md 8(b): a global alias next to the drivers' `using namespace
    sparsifyme;` would make `sparsify<2,2>(...)` ambiguous).  tests/cpp/alias_parity reaches every operator through the alias and holds
    its values against the oracle; spmma() must return three non-zero stage times (the default since round 6)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp")], check=True, capture_output=True)
    out = subprocess.run([os.path.join(root, "tests", "cpp", "bin", "alias_parity")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "MISMATCH" not in out.stdout and out.stdout.count(": ok") == 6 and "6 checks, 0 failed" in out.stdout


# ---------------------------------------------------------------------------------------------
# (f-2) transposed operands of spmma (reference spmma.hxx:30-31,67-69)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", [(196, 64, 128, 2), (130, 72, 200, 3), (64, 64, 64, 1), (77, 40, 36, 2)])
@pytest.mark.parametrize("tatb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_spmma_transposed_operands_vs_oracle(gpu, orc, dtype, shape, tatb):
    """The sequence include/sparsify.me/spmma.hxx runs for (transpose_a, transpose_b), through the C ABI: stored A is
    k x m (ta) / stored B is n x k (tb), row-major contiguous; sm_transpose -> TILE prune -> transpose back (A ends
    pruned in place) -> compress -> multiply.  Oracle: numpy transposes around the oracle's prune / compress / spmma."""
    import torch
    m, n, k, batch = shape
    ta, tb = tatb
    rng = np.random.default_rng(m + 3 * n + 5 * k + 7 * ta + 11 * tb)
    A = rand(rng, batch * m * k, dtype).reshape(batch, m, k)      # op(A)
    B = rand(rng, batch * k * n, dtype).reshape(batch, k, n)      # op(B)
    storedA = np.ascontiguousarray(A.transpose(0, 2, 1)) if ta else A.copy()
    storedB = np.ascontiguousarray(B.transpose(0, 2, 1)) if tb else B.copy()
    dA, dB = to_dev(storedA.reshape(-1)), to_dev(storedB.reshape(-1))
    es = A.dtype.itemsize
    if ta:
        An = torch.empty_like(dA)
        gpu.transpose(dA, An, k, m, batch=batch)
    else:
        An = dA
    for b in range(batch):   # per batch: m need not be a multiple of 4 (a TILE must not straddle two batches)
        seg = An[b * m * k:(b + 1) * m * k]
        gpu.prune24(seg, seg, m, k, k, gpu.PRUNE_TILE)
    if ta:
        gpu.transpose(An, dA, m, k, batch=batch)
    blob = torch.empty(gpu.compress24_size(m, k, es, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(An, m, k, k, batch, m * k, blob)
    if tb:
        Bn = torch.empty_like(dB)
        gpu.transpose(dB, Bn, n, k, batch=batch)
    else:
        Bn = dB
    C = torch.zeros(batch * m * n, dtype=torch_dtype(dtype), device="cuda")
    gpu.spmma(blob, Bn, C, m, n, k, batch, k * n)
    # oracle
    P = np.stack([orc.prune24(bits(A[b].reshape(-1)), m, k, k, orc.TILE).view(dtype).reshape(m, k) for b in range(batch)])
    wantA = np.ascontiguousarray(P.transpose(0, 2, 1)) if ta else P
    assert np.array_equal(bits(host(dA)), bits(wantA.reshape(-1))), "stored A is not the TILE-pruned operand in place"
    ob = orc.compress24(bits(P.reshape(-1)), m, k, k, batch)
    assert np.array_equal(host(blob), ob)
    Cref = np.zeros(batch * m * n, dtype=bits(A.reshape(-1)).dtype if es == 2 else np.float32)
    orc.spmma(ob, bits(B.reshape(-1)) if es == 2 else B.reshape(-1), Cref, m, n, k, batch, k * n)
    scale = np.stack([np.abs(P[b].astype(np.float64)) @ np.abs(B[b].astype(np.float64)) for b in range(batch)]).reshape(-1)
    if es == 2:
        check_close(host(C), Cref.view(np.float16), scale, FP16_TOL, f"spmma ta={ta} tb={tb} {shape}", k)
    else:
        check_close(host(C), Cref, scale, FP32_TOL, f"spmma_f32 ta={ta} tb={tb} {shape}", k, "f32")


@pytest.mark.parametrize("es,npdt", [(2, np.uint16), (4, np.uint32), (8, np.uint64)])
def test_transpose_bit_exact_with_leading_dimensions(gpu, es, npdt):
    import torch
    rng = np.random.default_rng(es)
    for (rows, cols, ld_in, ld_out, batch) in [(1, 1, 1, 1, 1), (64, 64, 64, 64, 2), (77, 130, 136, 80, 3), (200, 3, 5, 200, 1), (3, 1000, 1000, 8, 2)]:
        src = rng.integers(0, 2 ** 16, batch * rows * ld_in).astype(npdt)
        dst0 = rng.integers(0, 2 ** 16, batch * cols * ld_out).astype(npdt)
        tdt = {2: torch.int16, 4: torch.int32, 8: torch.int64}[es]
        dsrc = torch.from_numpy(src.view({2: np.int16, 4: np.int32, 8: np.int64}[es])).cuda()
        ddst = torch.from_numpy(dst0.view({2: np.int16, 4: np.int32, 8: np.int64}[es]).copy()).cuda()
        assert dsrc.dtype == tdt
        gpu.transpose(dsrc, ddst, rows, cols, ld_in, ld_out, batch)
        want = dst0.copy().reshape(batch, cols, ld_out)
        want[:, :, :rows] = src.reshape(batch, rows, ld_in)[:, :, :cols].transpose(0, 2, 1)   # padding columns untouched
        assert np.array_equal(host(ddst).view(npdt), want.reshape(-1))
    with pytest.raises(gpu.SparsifymeError):
        gpu.transpose(dsrc, dsrc, 4, 4)   # in place is refused


# ---------------------------------------------------------------------------------------------
# (f-1) fused prune -> compress -> matmul
# ---------------------------------------------------------------------------------------------
# the form every row of test_fused_equals_staged runs on an MI355X (256 CUs), shared and per-batch B alike; pinned without a GPU by
# tests/test_fused_form_abi.py
FUSED_ROW_FORMS = {(128, 64, 64, 1): "direct64", (196, 512, 256, 2): "astat", (784, 256, 1024, 2): "widep", (130, 72, 192, 1): "direct128",
                   (96, 64, 128, 3): "direct64", (12544, 64, 576, 2): "direct64", (3136, 128, 1152, 1): "direct128_nt", (300, 136, 320, 2): "widep",
                   (300, 520, 128, 2): "astat", (784, 1024, 256, 1): "astat", (130, 2048, 512, 1): "astat", (4000, 264, 64, 1): "astat",
                   (260, 520, 576, 1): "widep", (3136, 256, 192, 12): "big", (2200, 264, 320, 16): "astat", (3000, 256, 128, 11): "big",
                   (260, 520, 1088, 1): "wide", (3190, 256, 192, 24): "widep", (4785, 200, 320, 16): "widep", (3000, 256, 128, 26): "widep"}


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 512, 256, 2), (784, 256, 1024, 2), (130, 72, 192, 1), (96, 64, 128, 3),
                                   (12544, 64, 576, 2), (3136, 128, 1152, 1), (300, 136, 320, 2),
                                   # A-stationary kernel (n > 256, k <= 512): column tails, row tails, single stage, 8 stages
                                   (300, 520, 128, 2), (784, 1024, 256, 1), (130, 2048, 512, 1), (4000, 264, 64, 1),
                                   # persistent wide kernel with several column tiles (n > 256, 512 < k <= 1024)
                                   (260, 520, 576, 1),
                                   # many-tile launches of the big form (its rounds fill the chip as well as the 128-row kernels') and of
                                   # the A-stationary kernel: odd stage counts, ragged rows / columns
                                   (3136, 256, 192, 12), (2200, 264, 320, 16), (3000, 256, 128, 11),
                                   # wide kernel beyond its one-tile range (n > 256, k > 1024)
                                   (260, 520, 1088, 1),
                                   # persistent wide kernel with more tiles than CUs (599-624 tiles of 128 rows against 300-312 of 256: a
                                   # workgroup walks 2-3 tiles): an odd stage count (the A image's buffer parity flips between tiles),
                                   # ragged rows / columns
                                   (3190, 256, 192, 24), (4785, 200, 320, 16), (3000, 256, 128, 26)])
@pytest.mark.parametrize("shared_b", [True, False])
def test_fused_equals_staged(gpu, orc, shape, shared_b):
    """sm_spmma_fused_f16(A) must be BIT-identical to sm_spmma_f16(sm_compress24_f16(A)): same kept values,
    same position codes, same instruction sequence; and (tolerance) match the oracle.  The form each row is there for is asserted
    through sm_spmma_fused_form on this device (FUSED_ROW_FORMS)."""
    import torch
    m, n, k, batch = shape
    assert gpu.spmma_fused_form(m, n, k, batch=batch, strideB=0 if shared_b else k * n) == FUSED_ROW_FORMS[shape], f"{shape} reaches another form on this device"
    rng = np.random.default_rng(m * 3 + n + k * 5)
    A = rand(rng, batch * m * k, np.float16, "ties" if m % 7 == 0 else "uniform")
    nb = 1 if shared_b else batch
    B = rand(rng, nb * k * n, np.float16)
    strideB = 0 if shared_b else k * n
    dA, dB = to_dev(A), to_dev(B)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    C1 = torch.zeros(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, C1, m, n, k, batch, strideB)
    C2 = torch.full((batch * m * n,), 7.0, dtype=torch.float16, device="cuda")
    gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch, strideB=strideB)
    assert np.array_equal(bits(host(C1)), bits(host(C2))), "fused result differs from compress + spmma"
    ob = orc.compress24(bits(A), m, k, k, batch)
    Cref = np.zeros(batch * m * n, dtype=np.uint16)
    orc.spmma(ob, bits(B), Cref, m, n, k, batch, strideB)
    scale = np.stack([np.abs(A.astype(np.float64)).reshape(batch, m, k)[b] @ np.abs(B.astype(np.float64)).reshape(nb, k, n)[b if not shared_b else 0]
                      for b in range(batch)]).reshape(-1)
    check_close(host(C2), Cref.view(np.float16), scale, FP16_TOL, f"fused {shape}", k)


@pytest.mark.parametrize("shape", [(2045, 256, 128, 32), (2045, 264, 576, 32), (2048, 512, 576, 32), (128, 256, 128, 1), (100, 264, 576, 1)],
                         ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_fused_big_form_equals_staged(gpu, shape, bf):
    """The 256-row BIG form of the fused kernel (round 4; spmma_f16_fused.hip: spmma_f16_fused_big_kernel), which the dispatch
    takes for n > 128 when its one-per-CU workgroups fill the chip's rounds at least as well as the 128-row kernels' -- here:
    65 440 / 65 536 stacked rows = 256 big tiles against 512 (a ragged last tile, one and two column tiles, a column tail), and
    single-tile problems -- against sm_compress24 + sm_spmma, bit for bit: shared and per-batch B, alpha / beta != (1, 0),
    grouped launches of three."""
    import torch
    m, n, k, batch = shape
    tdt = torch.bfloat16 if bf else torch.float16
    dA = torch.empty(batch * m * k, dtype=tdt, device="cuda")
    gpu.fill_uniform(dA, 0xB16 + m + n, -1.0, 1.0)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    for shared_b, (alpha, beta) in ((True, (1.0, 0.0)), (False, (1.0, 0.0)), (True, (0.5, -2.0))):
        nb = 1 if shared_b else batch
        dB = torch.empty(nb * k * n, dtype=tdt, device="cuda")
        gpu.fill_uniform(dB, 0xB17 + k, -1.0, 1.0)
        strideB = 0 if shared_b else k * n
        assert gpu.spmma_fused_form(m, n, k, batch=batch, strideB=strideB, beta=beta) == "big", f"{shape} (shared_b={shared_b}, beta={beta}) reaches another form"
        C0 = torch.empty(batch * m * n, dtype=tdt, device="cuda")
        gpu.fill_uniform(C0, 0xC17, -1.0, 1.0)
        C1, C2 = C0.clone(), C0.clone()
        gpu.spmma(blob, dB, C1, m, n, k, batch, strideB, alpha=alpha, beta=beta)
        gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch, strideB=strideB, alpha=alpha, beta=beta)
        assert torch.equal(C1.view(torch.int16), C2.view(torch.int16)), f"big form differs from compress + spmma (shared_b={shared_b}, alpha={alpha}, beta={beta})"
    # grouped: three problems in one grid
    As = [dA] + [torch.empty_like(dA) for _ in range(2)]
    for i in (1, 2):
        gpu.fill_uniform(As[i], 0xB20 + i, -1.0, 1.0)
    Bs = [torch.empty(k * n, dtype=tdt, device="cuda") for _ in range(3)]
    for i, B_ in enumerate(Bs):
        gpu.fill_uniform(B_, 0xB30 + i, -1.0, 1.0)
    Cs = [torch.full((batch * m * n,), float("nan"), dtype=tdt, device="cuda") for _ in range(3)]
    assert gpu.spmma_fused_form(m, n, k, batch=batch, count=3) == "big"
    gpu.spmma_fused_grouped(As, Bs, Cs, m, n, k, batch=batch)
    Cref = torch.empty(batch * m * n, dtype=tdt, device="cuda")
    for i in range(3):
        gpu.compress24(As[i], m, k, k, batch, m * k, blob)
        gpu.spmma(blob, Bs[i], Cref, m, n, k, batch)
        assert torch.equal(Cs[i].view(torch.int16), Cref.view(torch.int16)), f"grouped big form, problem {i}"


@pytest.mark.parametrize("shape", [(196, 512, 2048, 4), (100, 264, 2304, 3), (300, 256, 2304, 2), (64, 136, 4608, 1), (600, 512, 3072, 5)], ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
def test_fused_streamk_vs_oracle(gpu, orc, shape, bf, ab):
    """The STREAM-K form of the fused kernel (round 5: sm_spmma_fused_*_ws -> spmma_f16_fused_sk_kernel): few 256 x 256 tiles with a
    long K, so every tile is cut into several slot ranges (2-9 stages per workgroup: up to seven partial sums meet in one tile's fix-up;
    groups of several panels with a partial last group: the full-size test below), ragged rows and columns, shared B, alpha / beta.  Held against the ORACLE's compress -> spmma inside the tight bound
    (one rounding + k fp32 accumulation steps): the order of a cut tile's fp32 additions differs from the staged kernels', nothing
    else does.  Twice: the second run must give the same bits (fixed-order fix-up, no atomics on data), and the flags are zero again."""
    import torch
    m, n, k, batch = shape
    alpha, beta = ab
    rng = np.random.default_rng(m + 2 * n + 3 * k + 7 * bf)
    if bf:
        A, Bm, C0 = bf16_bits(rng, batch * m * k), bf16_bits(rng, k * n), bf16_bits(rng, batch * m * n)
        dA, dB = bf16_dev(A), bf16_dev(Bm)
        mk = bf16_dev
    else:
        A, Bm, C0 = bits(rand(rng, batch * m * k, np.float16)), bits(rand(rng, k * n, np.float16)), bits(rand(rng, batch * m * n, np.float16))
        mk = lambda x: torch.from_numpy(x.view(np.int16)).cuda().view(torch.float16)
        dA, dB = mk(A), mk(Bm)
    ws = _sk_ws(gpu)
    C1 = mk(C0.copy())
    gpu.spmma_fused(dA, dB, C1, m, n, k, batch=batch, alpha=alpha, beta=beta, workspace=ws)
    torch.cuda.synchronize()
    assert _sk_ran(ws), "the shape was meant to take the stream-K kernel"
    assert bool((ws[:4096] == 0).all().item()), "flags not handed back as zero"
    assert gpu.spmma_fused_workspace_state(ws) == 0
    C2 = mk(C0.copy())
    gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch, alpha=alpha, beta=beta, workspace=ws)
    assert torch.equal(C1.view(torch.int16), C2.view(torch.int16)), "stream-K result differs between two runs"
    assert gpu.spmma_fused_workspace_state(ws) == 0
    ob = orc.compress24(A, m, k, k, batch)
    Cref = C0.copy()
    kw = dict(alpha=alpha, beta=beta)
    if bf:
        orc.spmma(ob, Bm, Cref, m, n, k, batch, 0, bf16=True, **kw)
        pruned = orc.prune24(A, batch * m, k, k, orc.STRIP, bf16=True)
        scale = abs(alpha) * (np.abs(bf16_f64(pruned)).reshape(batch * m, k) @ np.abs(bf16_f64(Bm)).reshape(k, n)).reshape(-1) + abs(beta) * np.abs(bf16_f64(C0))
        check_close(bf16_f64(bf16_host(C1)), bf16_f64(Cref), scale, FP16_TOL, f"stream-K bf16 {shape}", k, "bf16")
    else:
        orc.spmma(ob, Bm, Cref, m, n, k, batch, 0, **kw)
        P = np.abs(orc.decompress24(ob, m, k, k, np.uint16, batch=batch).view(np.float16).astype(np.float64)).reshape(batch * m, k)
        scale = abs(alpha) * (P @ np.abs(Bm.view(np.float16).astype(np.float64)).reshape(k, n)).reshape(-1) + abs(beta) * np.abs(C0.view(np.float16).astype(np.float64))
        check_close(host(C1), Cref.view(np.float16), scale, FP16_TOL, f"stream-K {shape}", k)


def test_fused_workspace_state_reports_a_dirty_flag_page(gpu):
    """sm_spmma_fused_workspace_state: 0 for a clean page, 1 when the timeout word (1023) is set, 2 for raised flags without
    it -- what a caller (and bench.py, after its timed loop) asks before trusting a stream-K launch's C or reusing the workspace."""
    import torch
    ws = gpu.spmma_fused_workspace()
    assert gpu.spmma_fused_workspace_state(ws) == 0
    flags = ws[:4096].view(torch.int32)
    flags[17] = 1
    assert gpu.spmma_fused_workspace_state(ws) == 2
    flags[1023] = 0xdead
    assert gpu.spmma_fused_workspace_state(ws) == 1
    flags.zero_()
    assert gpu.spmma_fused_workspace_state(ws) == 0


def test_conv_spmma_workspace_covers_w224_with_a_4_byte_aligned_x(gpu):
    """a geometry only the 16-byte patch plan takes (W % 8 == 0, W + border > 128 halves: W = 224) with an X that is only
    4-byte aligned -- the workspace query must size the blob for it, and sm_conv_spmma_* must then run (the pair) instead of returning
    NOT_SUPPORTED; the result equals the aligned call's bit for bit."""
    import torch
    N, Cin, H, W, n_out = 1, 8, 16, 224, 64
    need = gpu.conv_spmma_workspace(N, Cin, H, W, 3, 3, 1, 1, 1)
    assert need > 0
    Xbuf = torch.empty(N * Cin * H * W + 8, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(Xbuf, 0x224, -1.0, 1.0)
    X4 = Xbuf[2:2 + N * Cin * H * W]          # 4-byte aligned, not 16
    X16 = X4.clone()
    B = torch.empty(Cin * 9 * n_out, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(B, 0x225, -1.0, 1.0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    C4 = torch.empty(N * H * W * n_out, dtype=torch.float16, device="cuda")
    C16 = torch.empty_like(C4)
    gpu.conv_spmma(X4, B, C4, N, Cin, H, W, 3, 3, 1, 1, 1, n_out, workspace=ws)
    gpu.conv_spmma(X16, B, C16, N, Cin, H, W, 3, 3, 1, 1, 1, n_out, workspace=ws)
    assert torch.equal(C4.view(torch.int16), C16.view(torch.int16))


@pytest.mark.parametrize("case", [(196, 512, 4608, 32, 3), (196, 512, 4608, 32, 1), (784, 256, 4608, 32, 3)], ids=lambda c: "x".join(map(str, c)))
def test_fused_streamk_full_size_properties(gpu, case):
    """The ResNet-50 shapes the stream-K form serves, as bench.py launches them (b = 32, the table's instance count, grouped, one
    workspace): (i) every tile that lies whole inside one workgroup's range of stage units equals the no-workspace result BIT FOR
    BIT (that result equals compress + spmma, which is held against the oracle); (ii) every other element is within one fp16
    rounding + the fp32 accumulation bound of it (the fp64 product of the STRIP-pruned operand on the device gives the scale);
    (iii) two runs give the same bits; (iv) the flags are zero again."""
    import torch
    m, n, k, batch, cnt = case
    As, Bs, Cb, Cw = [], [], [], []
    for i in range(cnt):
        A = torch.empty(batch * m * k, dtype=torch.float16, device="cuda"); gpu.fill_uniform(A, 0x51 + i, -1.0, 1.0)
        B_ = torch.empty(k * n, dtype=torch.float16, device="cuda"); gpu.fill_uniform(B_, 0x61 + i, -1.0, 1.0)
        As.append(A); Bs.append(B_)
        Cb.append(torch.full((batch * m * n,), float("nan"), dtype=torch.float16, device="cuda"))
        Cw.append(torch.full((batch * m * n,), float("nan"), dtype=torch.float16, device="cuda"))
    ws = _sk_ws(gpu)
    gpu.spmma_fused_grouped(As, Bs, Cb, m, n, k, batch=batch)
    gpu.spmma_fused_grouped(As, Bs, Cw, m, n, k, batch=batch, workspace=ws)
    torch.cuda.synchronize()
    assert _sk_ran(ws) and bool((ws[:4096] == 0).all().item())
    Cw2 = [torch.full_like(c, float("nan")) for c in Cw]
    gpu.spmma_fused_grouped(As, Bs, Cw2, m, n, k, batch=batch, workspace=ws)
    for x, y in zip(Cw, Cw2):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), "two stream-K runs differ"
    # the decomposition the kernel uses, from the library itself: row panels (256 rows of a problem, problem order) x nkt stage units
    M = m * batch
    tm, tn, nkt = (M + 255) // 256, (n + 255) // 256, k // 64
    takes, plan = gpu.spmma_fused_streamk_plan(M, n, k, cnt)
    assert takes and plan["wg"] > 1
    whole = set(gpu.streamk_whole_panels(plan, cnt * tm, nkt))
    assert len(whole) < cnt * tm, "the plan was meant to cut some tiles"
    for i in range(cnt):
        base, got = Cb[i].view(M, n), Cw[i].view(M, n)
        for r in range(tm):
            if i * tm + r in whole:
                b_, g_ = base[r * 256:(r + 1) * 256], got[r * 256:(r + 1) * 256]
                assert torch.equal(b_.view(torch.int16), g_.view(torch.int16)), f"whole row panel {i * tm + r} differs from the no-workspace result"
        # (ii) all elements: |got - fp64 product| <= one fp16 rounding + k accumulation steps
        P = As[i].clone()
        gpu.prune24(P, P, M, k, k, gpu.PRUNE_STRIP)
        P64, B64 = P.view(M, k).double(), Bs[i].view(k, n).double()
        ref, scale = P64 @ B64, P64.abs() @ B64.abs()
        bound = ROUND["f16"] * ref.abs() + 2.0 * k * ACC["f16"] * scale + TINY["f16"]
        ratio = float(((got.double() - ref).abs() / bound).max().item())
        MARGINS.append((f"stream-K full size {case} problem {i}", ratio))
        assert ratio <= 1.0, f"stream-K {case} problem {i}: max err / bound = {ratio:.3f}"
        del P, P64, B64, ref, scale, bound


@pytest.mark.parametrize("shape", [(3136, 512, 128, 24), (2100, 264, 256, 32), (4096, 384, 64, 17), (2049, 520, 192, 32)])
def test_fused_astat_many_panels_equals_staged(gpu, shape):
    """The A-stationary kernel at grouped-launch sizes (several rounds of row panels per CU; one- to four-stage panels, ragged
    rows and columns) must return the bits of sm_compress24 + sm_spmma.  (The staged pair is the one held against the
    oracle, test_spmma_f16_vs_oracle; at these sizes the CPU product would take minutes.)"""
    import torch
    m, n, k, batch = shape
    assert gpu.spmma_fused_form(m, n, k, batch=batch) == "astat" and gpu.spmma_fused_form(m, n, k, batch=batch, count=2) == "astat", f"{shape} reaches another form"
    dA = torch.empty(batch * m * k, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dA, 1234 + m, -1.0, 1.0)
    dB = torch.empty(k * n, dtype=torch.float16, device="cuda")
    gpu.fill_uniform(dB, 4321 + n, -1.0, 1.0)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    C1 = torch.zeros(batch * m * n, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, C1, m, n, k, batch, 0)
    C2 = torch.full((batch * m * n,), 7.0, dtype=torch.float16, device="cuda")
    gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch)
    torch.cuda.synchronize()
    assert torch.equal(C1.view(torch.int16), C2.view(torch.int16)), "A-stationary result differs from compress + spmma"
    # and as a grouped launch of two problems
    dA2 = torch.roll(dA, 3)
    Cs = [torch.full((batch * m * n,), 5.0, dtype=torch.float16, device="cuda") for _ in range(2)]
    gpu.spmma_fused_grouped([dA, dA2], [dB, dB], Cs, m, n, k, batch=batch)
    C3 = torch.zeros_like(C1)
    gpu.spmma_fused(dA2, dB, C3, m, n, k, batch=batch)
    torch.cuda.synchronize()
    assert torch.equal(Cs[0].view(torch.int16), C1.view(torch.int16)) and torch.equal(Cs[1].view(torch.int16), C3.view(torch.int16))


@pytest.mark.parametrize("shape", [(12544, 64, 147, 2), (196, 64, 147, 3), (196, 64, 147, 4), (130, 128, 72, 2), (77, 24, 8, 4), (300, 72, 200, 1),
                                   (513, 64, 100, 1), (520, 64, 100, 1), (128, 64, 333, 2), (40, 128, 190, 2)])
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_fused_span_form_equals_staged(gpu, orc, shape, bf):
    """k % 64 != 0 (the 7 x 7 x 3 stem layer, k = 147, and other ragged depths): sm_spmma_fused_* now runs the span form
    (a tile's rows as one contiguous byte span through LDS) and must return the bits of sm_compress24 + sm_spmma -- ragged
    last strip completed with virtual zeros, B rows at or beyond k from a zero page (inf / NaN in the clamped neighbourhood
    must not leak), partial last tile, stacked batches; plus the grouped entry on the same shapes."""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + 3 * n + 7 * k + bf)
    if bf:
        A = bf16_bits(rng, batch * m * k, "ties" if m % 2 else "uniform")
        B = bf16_bits(rng, k * n)
        dA, dB = bf16_dev(A), bf16_dev(B)
        tdt = torch.bfloat16
        hostbits = bf16_host
    else:
        Af = rand(rng, batch * m * k, np.float16, "ties" if m % 2 else "uniform")
        Af[:4] = np.array([np.inf, -np.inf, 65504.0, -65504.0], dtype=np.float16)   # large values next to the k tail of row 0
        A, B = bits(Af), bits(rand(rng, k * n, np.float16))
        dA, dB = to_dev(Af), to_dev(B.view(np.float16))
        tdt = torch.float16
        hostbits = lambda t: bits(host(t))
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    C1 = torch.zeros(batch * m * n, dtype=tdt, device="cuda")
    gpu.spmma(blob, dB, C1, m, n, k, batch, 0)
    C2 = torch.full((batch * m * n,), 7.0, dtype=tdt, device="cuda")
    for cnt in (1, 3):
        assert gpu.spmma_fused_form(m, n, k, batch=batch, count=cnt) == ("not_taken" if (batch * m * k) % 8 else "span"), f"{shape} reaches another form"
    if (batch * m * k) % 8:   # the operand does not end on a 16-byte boundary: the span form declines (its last DMA piece
        with pytest.raises(gpu.SparsifymeError, match="status 2"):   # would read past the buffer); callers take the staged pair
            gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch)
        return
    gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch)
    assert np.array_equal(hostbits(C1), hostbits(C2)), "span-form fused result differs from compress + spmma"
    # grouped: three problems, the middle one the data above
    dA0, dA2 = torch.roll(dA, 5), torch.roll(dA, 11)
    Cs = [torch.full((batch * m * n,), 3.0, dtype=tdt, device="cuda") for _ in range(3)]
    gpu.spmma_fused_grouped([dA0, dA, dA2], [dB, dB, dB], Cs, m, n, k, batch=batch)
    assert np.array_equal(hostbits(Cs[1]), hostbits(C1))
    for a_, c_ in ((dA0, Cs[0]), (dA2, Cs[2])):
        cw = torch.zeros(batch * m * n, dtype=tdt, device="cuda")
        gpu.spmma_fused(a_, dB, cw, m, n, k, batch=batch)
        assert np.array_equal(hostbits(cw), hostbits(c_))
    if not bf and np.isfinite(A.view(np.float16).astype(np.float32)).all():
        ob = orc.compress24(A, m, k, k, batch)
        Cref = np.zeros(batch * m * n, dtype=np.uint16)
        orc.spmma(ob, B, Cref, m, n, k, batch, 0)
        assert np.array_equal(Cref, Cref)  # (the oracle comparison of the staged pair lives in test_spmma_f16_vs_oracle)


@pytest.mark.parametrize("shape", [(196, 64, 128, 2), (784, 256, 1024, 1), (300, 520, 128, 2), (260, 520, 576, 1), (3136, 128, 512, 1),
                                   (130, 72, 192, 1), (3136, 256, 192, 2)])
@pytest.mark.parametrize("count", [1, 3, 8, 11])
def test_fused_grouped_equals_individual_calls(gpu, shape, count):
    """sm_spmma_fused_f16_grouped over `count` same-shape problems (one grid per 8) writes, into every C[i], exactly the bits
    of a plain sm_spmma_fused_f16 call on (A[i], B[i]) -- every kernel variant (direct, wide, A-stationary), ragged tiles,
    more problems than one launch holds.  bf16 rides the same kernels (one case)."""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(count * 1000 + m + n + k)
    As = [to_dev(rand(rng, batch * m * k, np.float16, "ties" if i % 3 == 2 else "uniform")) for i in range(count)]
    Bs = [to_dev(rand(rng, k * n, np.float16)) for _ in range(count)]
    want = []
    for i in range(count):
        C = torch.full((batch * m * n,), 3.0, dtype=torch.float16, device="cuda")
        gpu.spmma_fused(As[i], Bs[i], C, m, n, k, batch=batch)
        want.append(bits(host(C)))
    Cs = [torch.full((batch * m * n,), 5.0, dtype=torch.float16, device="cuda") for _ in range(count)]
    gpu.spmma_fused_grouped(As, Bs, Cs, m, n, k, batch=batch)
    for i in range(count):
        assert np.array_equal(bits(host(Cs[i])), want[i]), f"grouped problem {i} of {count} differs from its own call"
    if count == 3:
        Ab = [a.view(torch.int16).view(torch.bfloat16) for a in As]
        Bb = [b.view(torch.int16).view(torch.bfloat16) for b in Bs]
        Cb = [torch.zeros(batch * m * n, dtype=torch.bfloat16, device="cuda") for _ in range(count)]
        gpu.spmma_fused_grouped(Ab, Bb, Cb, m, n, k, batch=batch)
        for i in range(count):
            C = torch.zeros(batch * m * n, dtype=torch.bfloat16, device="cuda")
            gpu.spmma_fused(Ab[i], Bb[i], C, m, n, k, batch=batch)
            torch.cuda.synchronize()
            assert torch.equal(C.view(torch.int16), Cb[i].view(torch.int16))


@pytest.mark.parametrize("shape", [(196, 64, 128, 2), (784, 256, 1024, 1), (300, 520, 128, 2), (196, 512, 1152, 4), (3136, 128, 512, 1), (130, 72, 192, 1),
                                   (131, 70, 100, 2), (12544, 64, 64, 1)], ids=lambda s_: "x".join(map(str, s_)))
@pytest.mark.parametrize("count", [1, 3, 8, 11])
def test_spmma_grouped_equals_individual_calls(gpu, shape, count):
    """sm_spmma_f16_grouped over `count` same-shape compressed operands (one grid per 8) writes, into every C[i], exactly the bits of
    a plain sm_spmma_f16 call on (blob[i], B[i]) -- every staged kernel (DMA, producer / consumer, the 256-row tile, the predicated
    fall-back for ragged shapes), alpha / beta, more problems than one launch holds; bf16 rides the same kernels (one case)."""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(count * 77 + m + n + k)
    blobs, Bs, want = [], [], []
    for i in range(count):
        A = to_dev(rand(rng, batch * m * k, np.float16, "ties" if i % 3 == 2 else "uniform"))
        blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
        gpu.compress24(A, m, k, k, batch, m * k, blob)
        blobs.append(blob)
        Bs.append(to_dev(rand(rng, k * n, np.float16)))
    for (alpha, beta) in [(1.0, 0.0), (0.5, -2.0)]:
        want = []
        for i in range(count):
            C = torch.full((batch * m * n,), 3.0, dtype=torch.float16, device="cuda")
            gpu.spmma(blobs[i], Bs[i], C, m, n, k, batch, alpha=alpha, beta=beta)
            want.append(bits(host(C)))
        Cs = [torch.full((batch * m * n,), 3.0, dtype=torch.float16, device="cuda") for _ in range(count)]
        gpu.spmma_grouped(blobs, Bs, Cs, m, n, k, batch=batch, alpha=alpha, beta=beta)
        for i in range(count):
            assert np.array_equal(bits(host(Cs[i])), want[i]), f"grouped problem {i} of {count} differs from its own call (alpha {alpha}, beta {beta})"
    if count == 3:
        Bb = [b.view(torch.int16).view(torch.bfloat16) for b in Bs]
        Cb = [torch.zeros(batch * m * n, dtype=torch.bfloat16, device="cuda") for _ in range(count)]
        gpu.spmma_grouped(blobs, Bb, Cb, m, n, k, batch=batch)
        for i in range(count):
            C = torch.zeros(batch * m * n, dtype=torch.bfloat16, device="cuda")
            gpu.spmma(blobs[i], Bb[i], C, m, n, k, batch)
            torch.cuda.synchronize()
            assert torch.equal(C.view(torch.int16), Cb[i].view(torch.int16))


def test_spmma_grouped_rejects_bad_arguments(gpu):
    import ctypes
    import torch
    L = gpu.lib()
    blob = torch.zeros(gpu.compress24_size(128, 64, 2, 1), dtype=torch.uint8, device="cuda")
    B = torch.zeros(64 * 64, dtype=torch.float16, device="cuda")
    C = torch.zeros(128 * 64, dtype=torch.float16, device="cuda")
    tab = lambda *ts: (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])
    z = ctypes.c_void_p(0)
    assert L.sm_spmma_f16_grouped(2, tab(blob, 0), tab(B, B), tab(C, C), 128, 64, 64, 1, 0, 128 * 64, 1.0, 0.0, z) != 0   # a null blob in the table
    assert L.sm_spmma_f16_grouped(2, z, tab(B, B), tab(C, C), 128, 64, 64, 1, 0, 128 * 64, 1.0, 0.0, z) != 0               # no table
    assert L.sm_spmma_f16_grouped(0, z, z, z, 128, 64, 64, 1, 0, 128 * 64, 1.0, 0.0, z) == 0                               # nothing to do


def test_fused_grouped_rejects_bad_arguments(gpu):
    import ctypes
    import torch
    L = gpu.lib()
    A = torch.zeros(128 * 64, dtype=torch.float16, device="cuda")
    C = torch.zeros(128 * 64 + 8, dtype=torch.float16, device="cuda")
    tab = lambda *ts: (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])
    z = ctypes.c_void_p(0)
    # a null operand in the table
    assert L.sm_spmma_fused_f16_grouped(2, tab(A, 0), tab(A, A), tab(C, C), 128, 64, 64, 64, 1, 128 * 64, 0, 128 * 64, 1.0, 0.0, z) != 0
    # a misaligned C in a group of two
    assert L.sm_spmma_fused_f16_grouped(2, tab(A, A), tab(A, A), tab(C, C.data_ptr() + 2), 128, 64, 64, 64, 1, 128 * 64, 0, 128 * 64, 1.0, 0.0, z) != 0
    # count == 0 is a no-op
    assert L.sm_spmma_fused_f16_grouped(0, None, None, None, 128, 64, 64, 64, 1, 128 * 64, 0, 128 * 64, 1.0, 0.0, z) == 0


# ---------------------------------------------------------------------------------------------
# (f-2) bfloat16 forms of the 2:4 path
# ---------------------------------------------------------------------------------------------
def bf16_dev(b):
    import torch
    return torch.from_numpy(b.view(np.int16)).cuda().view(torch.bfloat16)


def bf16_host(t):
    import torch
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("shape", [(4, 4), (7, 10), (196, 512), (130, 147), (784, 64), (33, 8)])
@pytest.mark.parametrize("alg", ["TILE", "STRIP"])
def test_prune24_bf16_vs_oracle(gpu, orc, shape, alg):
    import torch
    m, k = shape
    rng = np.random.default_rng(m * 7 + k)
    for kind in ("uniform", "ties"):
        A = bf16_bits(rng, m * k, kind)
        dA = bf16_dev(A)
        out = torch.empty_like(dA)
        gpu.prune24(dA, out, m, k, k, getattr(gpu, "PRUNE_" + alg))
        want = orc.prune24(A, m, k, k, getattr(orc, alg), bf16=True)
        assert np.array_equal(bf16_host(out), want), f"prune24 bf16 {alg} {shape} {kind}"
        valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        gpu.prune24_check(out, m, k, k, valid)
        assert int(host(valid)[0]) == 0


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 512, 256, 2), (784, 256, 1024, 2), (130, 72, 200, 3), (12544, 64, 147, 1),
                                   (3136, 128, 1152, 1), (300, 520, 128, 2), (131, 35, 77, 2)])
@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -2.0)])
def test_spmma_bf16_vs_oracle(gpu, orc, shape, ab):
    """compress (bit-exact, the fp16 kernels on the same bits) + 2:4 matmul on v_smfmac_f32_16x16x64_bf16, and the
    bf16 dense kernel on the pruned operand."""
    import torch
    m, n, k, batch = shape
    alpha, beta = ab
    rng = np.random.default_rng(m + 3 * n + 5 * k)
    A, B, C0 = bf16_bits(rng, batch * m * k), bf16_bits(rng, k * n), bf16_bits(rng, batch * m * n)
    dA, dB = bf16_dev(A), bf16_dev(B)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    ob = orc.compress24(A, m, k, k, batch)
    assert np.array_equal(host(blob), ob)
    back = torch.empty_like(dA)
    gpu.decompress24(blob, m, k, k, batch, m * k, back)
    pruned = orc.prune24(A, batch * m, k, k, orc.STRIP, bf16=True)
    assert np.array_equal(bf16_host(back), pruned)
    dC = bf16_dev(C0.copy())
    gpu.spmma(blob, dB, dC, m, n, k, batch, 0, alpha=alpha, beta=beta)
    Cref = C0.copy()
    orc.spmma(ob, B, Cref, m, n, k, batch, 0, alpha=alpha, beta=beta, bf16=True)
    scale = abs(alpha) * (np.abs(bf16_f64(A)).reshape(batch * m, k) @ np.abs(bf16_f64(B)).reshape(k, n)).reshape(-1) \
        + abs(beta) * np.abs(bf16_f64(C0))
    check_close(bf16_f64(bf16_host(dC)), bf16_f64(Cref), scale, FP16_TOL, f"spmma_bf16 {shape}", k, "bf16")
    # dense bf16 kernel on the pruned operand: the same products
    dC2 = bf16_dev(C0.copy())
    gpu.gemm_rowmajor(bf16_dev(pruned), dB, dC2, m, n, k, batch=batch, alpha=alpha, beta=beta)
    check_close(bf16_f64(bf16_host(dC2)), bf16_f64(Cref), scale, FP16_TOL, f"gemm_rowmajor_bf16 {shape}", k, "bf16")


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 512, 256, 2), (784, 256, 1024, 2), (12544, 64, 576, 1), (3136, 128, 1152, 1),
                                   (300, 520, 128, 2), (784, 1024, 256, 1), (260, 520, 576, 1)])
def test_fused_bf16_equals_staged(gpu, orc, shape):
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m * 3 + n + k * 5)
    A, B = bf16_bits(rng, batch * m * k, "ties" if m % 7 == 0 else "uniform"), bf16_bits(rng, k * n)
    dA, dB = bf16_dev(A), bf16_dev(B)
    blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    C1 = torch.zeros(batch * m * n, dtype=torch.bfloat16, device="cuda")
    gpu.spmma(blob, dB, C1, m, n, k, batch, 0)
    C2 = torch.full((batch * m * n,), 7.0, dtype=torch.bfloat16, device="cuda")
    gpu.spmma_fused(dA, dB, C2, m, n, k, batch=batch)
    assert np.array_equal(bf16_host(C1), bf16_host(C2)), "fused bf16 result differs from compress + spmma"
    Cref = np.zeros(batch * m * n, dtype=np.uint16)
    orc.spmma(orc.compress24(A, m, k, k, batch), B, Cref, m, n, k, batch, 0, bf16=True)
    scale = (np.abs(bf16_f64(A)).reshape(batch * m, k) @ np.abs(bf16_f64(B)).reshape(k, n)).reshape(-1)
    check_close(bf16_f64(bf16_host(C2)), bf16_f64(Cref), scale, FP16_TOL, f"fused bf16 {shape}", k, "bf16")


def test_fill_uniform_bf16(gpu):
    import torch
    x = torch.empty(1 << 16, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(1 << 16, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(x, 42, -1.0, 3.0)
    gpu.fill_uniform(y, 42, -1.0, 3.0)
    assert torch.equal(x, y.to(torch.bfloat16))     # same counter-based stream, rounded once to nearest even


# ---------------------------------------------------------------------------------------------
# (f-2) int8 forms of the 2:4 path (bit-exact: integer arithmetic)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 4), (7, 10), (196, 512), (130, 147), (784, 64), (33, 17)])
def test_prune24_i8_vs_oracle(gpu, orc, shape):
    import torch
    m, k = shape
    rng = np.random.default_rng(m * 7 + k)
    for kind in ("full", "ties"):
        A = (rng.integers(-128, 128, m * k) if kind == "full" else rng.integers(-2, 3, m * k)).astype(np.int8)
        dA = to_dev(A)
        out = torch.empty_like(dA)
        gpu.prune24(dA, out, m, k, k, gpu.PRUNE_TILE)
        want_t = orc.prune24(A.view(np.uint8), m, k, k, orc.TILE).view(np.int8)
        assert np.array_equal(host(out), want_t), f"prune24 i8 TILE {shape} {kind}"
        gpu.prune24(dA, out, m, k, k, gpu.PRUNE_STRIP)
        want = orc.prune24(A.view(np.uint8), m, k, k, orc.STRIP).view(np.int8)
        assert np.array_equal(host(out), want), f"prune24 i8 {shape} {kind}"
        valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        gpu.prune24_check(out, m, k, k, valid)
        assert int(host(valid)[0]) == 0
        gpu.prune24_check(dA, m, k, k, valid)
        assert int(host(valid)[0]) == orc.prune24_check(A.view(np.uint8), m, k, k)


@pytest.mark.parametrize("shape", [(128, 64, 64, 1), (196, 512, 256, 2), (784, 256, 1024, 2), (130, 72, 192, 3), (12544, 64, 576, 1),
                                   (3136, 128, 1152, 1), (300, 520, 128, 2), (2, 8, 64, 1), (258, 35, 320, 2)])
@pytest.mark.parametrize("shared_b", [True, False])
def test_spmma_i8_vs_oracle(gpu, orc, shape, shared_b):
    """compress (bit-exact) + v_smfmac_i32_16x16x128_i8 matmul: the int32 result equals the oracle's exactly, on one- and
    two-plane tails (k = 64, 192, 320, 576), row / column tails, shared and per-batch B, with and without accumulation."""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + 3 * n + 5 * k)
    A = rng.integers(-128, 128, batch * m * k).astype(np.int8)
    A[rng.uniform(0, 1, A.size) < 0.2] = 0
    nb = 1 if shared_b else batch
    B = rng.integers(-128, 128, nb * n * k).astype(np.int8)           # [n][k] per batch
    sB = 0 if shared_b else n * k
    dA, dB = to_dev(A), to_dev(B)
    blob = torch.full((gpu.compress24_size(m, k, 1, batch),), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.compress24(dA, m, k, k, batch, m * k, blob)
    ob = orc.compress24(A.view(np.uint8), m, k, k, batch)
    assert np.array_equal(host(blob), ob)
    back = torch.empty_like(dA)
    gpu.decompress24(blob, m, k, k, batch, m * k, back)
    assert np.array_equal(host(back).view(np.uint8), orc.prune24(A.view(np.uint8), batch * m, k, k, orc.STRIP))
    C0 = rng.integers(-1000, 1000, batch * m * n).astype(np.int32)
    for acc in (False, True):
        dC = to_dev(C0.copy())
        gpu.spmma_i8(blob, dB, dC, m, n, k, batch, sB, accumulate=acc)
        Cref = C0.copy()
        orc.spmma_i8(ob, B, Cref, m, n, k, batch, sB, accumulate=acc)
        assert np.array_equal(host(dC), Cref), f"spmma_i8 {shape} shared={shared_b} accumulate={acc}"
    # fused form (dense A in, no blob): the same int32 result bit for bit
    dF = to_dev(C0.copy())
    gpu.spmma_fused_i8(dA, dB, dF, m, n, k, batch=batch, strideB=sB, accumulate=True)
    assert np.array_equal(host(dF), Cref), f"spmma_fused_i8 {shape} shared={shared_b}"
    # requantised int8 output: saturate(rne(scale * acc)), bit-exact against the oracle's fp32 arithmetic
    Cacc = np.zeros(batch * m * n, dtype=np.int32)
    orc.spmma_i8(ob, B, Cacc, m, n, k, batch, sB)
    for scale in (2.0 ** -8, 0.0123):
        dQ = torch.full((batch * m * n,), 77, dtype=torch.int8, device="cuda")
        gpu.spmma_i8_q(blob, dB, dQ, m, n, k, scale, batch, sB)
        assert np.array_equal(host(dQ), orc.requant_i8(Cacc, scale)), f"spmma_i8_q {shape} scale {scale}"
        dQ2 = torch.full((batch * m * n,), 77, dtype=torch.int8, device="cuda")
        gpu.spmma_fused_i8(dA, dB, dQ2, m, n, k, batch=batch, strideB=sB, scale=scale)
        assert torch.equal(dQ, dQ2), f"spmma_fused_i8_q {shape} scale {scale}"


def test_transpose_i8_then_spmma_matches_row_major_b(gpu, orc):
    """The reference's B is row-major k x n; sm_transpose_i8 makes the [n][k] operand sm_spmma_i8 takes."""
    import torch
    rng = np.random.default_rng(5)
    for (k, n) in [(64, 64), (200, 72), (1, 5), (130, 257)]:
        Bkn = rng.integers(-128, 128, (k, n)).astype(np.int8)
        dT = torch.zeros(n * k, dtype=torch.int8, device="cuda")
        gpu.transpose_i8(to_dev(Bkn.reshape(-1)), dT, k, n)
        assert np.array_equal(host(dT).reshape(n, k), Bkn.T)
    m, n, k = 130, 72, 192
    A = rng.integers(-128, 128, m * k).astype(np.int8)
    Bkn = rng.integers(-128, 128, (k, n)).astype(np.int8)
    blob = torch.empty(gpu.compress24_size(m, k, 1, 1), dtype=torch.uint8, device="cuda")
    gpu.compress24(to_dev(A), m, k, k, 1, m * k, blob)
    dT = torch.empty(n * k, dtype=torch.int8, device="cuda")
    gpu.transpose_i8(to_dev(Bkn.reshape(-1)), dT, k, n)
    dC = torch.zeros(m * n, dtype=torch.int32, device="cuda")
    gpu.spmma_i8(blob, dT, dC, m, n, k)
    P = orc.prune24(A.view(np.uint8), m, k, k, orc.STRIP).view(np.int8).reshape(m, k).astype(np.int64)
    assert np.array_equal(host(dC).reshape(m, n), P @ Bkn.astype(np.int64))


def test_spmma_i8_rejects_what_it_cannot_take(gpu):
    import torch
    blob = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    B = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    C = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_i8(blob, B, C, 16, 16, 100)       # k % 64 != 0
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_i8(blob, B, C, 15, 16, 64)        # odd m


# ---------------------------------------------------------------------------------------------
# (f-3) im2col front end
# ---------------------------------------------------------------------------------------------
IM2COL_CFGS = [(2, 3, 9, 11, 3, 3, 1, 1, 1), (1, 4, 12, 12, 7, 7, 2, 3, 1), (2, 5, 8, 8, 1, 1, 1, 0, 1), (1, 2, 10, 9, 3, 2, 2, 0, 2),
               (1, 3, 224, 224, 7, 7, 2, 3, 1),      # the stem: K = 147 (ragged rows, K tail in the blob)
               (2, 64, 56, 56, 3, 3, 1, 1, 1),       # K = 576
               (1, 256, 14, 14, 3, 3, 2, 1, 1),      # K = 2304, several channel chunks, 7 x 7 outputs
               (1, 520, 7, 7, 1, 1, 1, 0, 1),        # 1 x 1, C not a multiple of the chunk
               (3, 16, 33, 70, 3, 3, 1, 1, 1)]       # three column blocks, ragged last one


@pytest.mark.parametrize("cfg", IM2COL_CFGS)
@pytest.mark.parametrize("tdt", ["f16", "bf16"])
def test_im2col_and_fused_compress_vs_oracle(gpu, orc, cfg, tdt):
    import torch
    N, C, H, W, kh, kw, s, p, d = cfg
    rng = np.random.default_rng(sum(cfg))
    X = rng.integers(0, 1 << 16, N * C * H * W).astype(np.uint16) if tdt == "bf16" else bits(rand(rng, N * C * H * W, np.float16))
    X[(X & 0x7fff) > 0x7c00] = 0x3c00                  # no NaN payload games in the equality checks
    dX = bf16_dev(X) if tdt == "bf16" else to_dev(X.view(np.float16))
    OH, OW = gpu.conv_out_size(H, kh, s, p, d), gpu.conv_out_size(W, kw, s, p, d)
    assert (OH, OW) == (orc.conv_out_size(H, kh, s, p, d), orc.conv_out_size(W, kw, s, p, d))
    L, K = OH * OW, C * kh * kw
    want = orc.im2col(X, N, C, H, W, kh, kw, s, p, d)
    dA = torch.full((N * L * K,), 7.0, dtype=dX.dtype, device="cuda")
    gpu.im2col(dX, N, C, H, W, kh, kw, s, p, d, dA)
    got = bf16_host(dA) if tdt == "bf16" else bits(host(dA))
    assert np.array_equal(got, want), f"im2col {cfg}"
    # fused form: the blob of that A, never materialising it
    blob = torch.full((gpu.compress24_size(L, K, 2, N),), 0xAB, dtype=torch.uint8, device="cuda")
    gpu.im2col(dX, N, C, H, W, kh, kw, s, p, d, blob, compress=True)
    assert np.array_equal(host(blob), orc.compress24(want, L, K, K, N)), f"im2col_compress24 {cfg}"
    blob2 = torch.empty_like(blob)
    gpu.compress24(dA, L, K, K, N, L * K, blob2)
    assert torch.equal(blob, blob2)


def test_conv_as_im2col_2to4_matmul(gpu):
    """End to end: activations -> (im2col + 2:4 compress in one kernel) -> sm_spmma against the filters == conv2d of
    the activations with, per output pixel, the same two-of-four receptive-field elements dropped."""
    import torch
    N, C, H, W, Co, kh, s, p = 2, 32, 20, 20, 64, 3, 1, 1
    g = torch.Generator().manual_seed(3)
    X = torch.randn(N, C, H, W, generator=g).half()
    Wt = torch.randn(Co, C, kh, kh, generator=g).half()
    OH = gpu.conv_out_size(H, kh, s, p, 1)
    L, K = OH * OH, C * kh * kh
    dX, dB = X.cuda().reshape(-1), Wt.reshape(Co, K).t().contiguous().cuda().reshape(-1)     # B = filters^T: K x Co
    blob = torch.empty(gpu.compress24_size(L, K, 2, N), dtype=torch.uint8, device="cuda")
    gpu.im2col(dX, N, C, H, W, kh, kh, s, p, 1, blob, compress=True)
    dC = torch.empty(N * L * Co, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, dC, L, Co, K, N, 0)
    # reference: unfold on the CPU, prune each row 2:4 (top-2 magnitudes per strip, ties to the lower index), matmul
    A = torch.nn.functional.unfold(X.float(), kh, padding=p, stride=s).transpose(1, 2).reshape(N * L, K // 4, 4)
    order = torch.argsort(-A.abs(), dim=-1, stable=True)
    keep = torch.zeros_like(A, dtype=torch.bool).scatter_(-1, order[..., :2], True)
    ref = (A * keep).reshape(N * L, K).double() @ Wt.reshape(Co, K).t().double()
    got = dC.cpu().double().reshape(N * L, Co)
    scale = (A.abs().reshape(N * L, K).double() @ Wt.reshape(Co, K).t().abs().double())
    assert ((got - ref).abs() <= FP16_TOL * scale.clamp_min(1e-30)).all()


CONV_CASES = [  # N, Cin, H, W, kh, kw, stride, pad, dil, n_out
    (2, 64, 14, 14, 3, 3, 1, 1, 1, 64),      # 196 pixels: one full and one partial tile per image, 13 patch rows
    (2, 64, 28, 28, 3, 3, 1, 1, 1, 128),
    (1, 128, 56, 56, 3, 3, 1, 1, 1, 128),    # ResNet-50 conv3_x geometry
    (1, 64, 112, 112, 3, 3, 1, 1, 1, 64),    # one patch row per DMA instruction
    (2, 64, 28, 28, 3, 3, 2, 1, 1, 64),      # stride 2
    (2, 64, 14, 14, 1, 1, 1, 0, 1, 72),      # 1 x 1 on 14 x 14, n % 64 != 0: a stage's 64 channels x 11 rows need 88 DMA instructions > 48: declined (not for its window)
    (1, 64, 20, 20, 3, 3, 1, 2, 2, 64),      # dilation 2
    (1, 256, 14, 14, 3, 3, 1, 1, 1, 256),    # two column tiles
    (1, 64, 18, 18, 5, 5, 1, 2, 1, 64),      # 25 phases
    (1, 64, 30, 30, 7, 7, 2, 3, 1, 64),      # 49 phases, stride 2
    (3, 64, 6, 6, 3, 3, 1, 1, 1, 64),        # L = 36 < 128
    (1, 64, 10, 12, 3, 3, 1, 0, 1, 64),      # no padding, H != W
    (1, 64, 56, 8, 7, 1, 2, 0, 1, 64),       # a narrow image whose stage plan exceeds the 16-byte form's 16 DMA instructions (18): the 4-byte form runs it
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_conv_spmma_fused_equals_im2col_compress_spmma(gpu, orc, case, bf):
    """sm_conv_spmma_fused_* (implicit GEMM: the A operand is gathered from an activation patch in LDS) must be
    BIT-identical to sm_im2col_compress24_* + sm_spmma_* -- same kept values, same codes, same SMFMAC sequence -- and,
    through that pair, match the oracle (im2col restatement -> compress -> spmma, fp64 accumulation).  The 1 x 1 case of the list is declined
    (status 2) for the size of its stage plan, not for its window: tests/test_gpu_conv.py runs the 1 x 1 layers the kernel takes."""
    import torch
    N, Cin, H, W, kh, kw, s_, p_, d_, n_out = case
    rng = np.random.default_rng(Cin + H * 3 + kh * 7 + s_)
    OH, OW = gpu.conv_out_size(H, kh, s_, p_, d_), gpu.conv_out_size(W, kw, s_, p_, d_)
    L, K = OH * OW, Cin * kh * kw
    if bf:
        X, Bw = bf16_bits(rng, N * Cin * H * W, "ties" if H == 14 else "uniform"), bf16_bits(rng, K * n_out)
        dX, dB = bf16_dev(X), bf16_dev(Bw)
        tdt = torch.bfloat16
    else:
        X = bits(rand(rng, N * Cin * H * W, np.float16, "ties" if H == 14 else "uniform"))
        Bw = bits(rand(rng, K * n_out, np.float16))
        dX = torch.from_numpy(X.view(np.int16)).cuda().view(torch.float16)
        dB = torch.from_numpy(Bw.view(np.int16)).cuda().view(torch.float16)
        tdt = torch.float16
    blob = torch.empty(gpu.compress24_size(L, K, 2, N), dtype=torch.uint8, device="cuda")
    gpu.im2col(dX, N, Cin, H, W, kh, kw, s_, p_, d_, blob, compress=True)
    C1 = torch.zeros(N * L * n_out, dtype=tdt, device="cuda")
    gpu.spmma(blob, dB, C1, L, n_out, K, N, 0)
    C2 = torch.full((N * L * n_out,), 7.0, dtype=tdt, device="cuda")
    if kh * kw == 1:
        # a 1 x 1 window makes a 64-deep stage touch 64 channels: on this 14 x 14 image that is nch * RI = 64 * 11 patch rows, 8 per DMA
        # instruction = 88 instructions against the plan's limit of 48.  THAT declines the case (sm_conv_spmma_fused_plan: "too many DMA
        # instructions"), and the documented pair above is the path; a smaller 1 x 1 layer is taken (tests/test_gpu_conv.py)
        with pytest.raises(gpu.SparsifymeError, match="status 2"):
            gpu.conv_spmma_fused(dX, dB, C2, N, Cin, H, W, kh, kw, s_, p_, d_, n_out)
        return
    gpu.conv_spmma_fused(dX, dB, C2, N, Cin, H, W, kh, kw, s_, p_, d_, n_out)
    torch.cuda.synchronize()
    assert torch.equal(C1.view(torch.int16), C2.view(torch.int16)), "implicit-GEMM result differs from im2col_compress24 + spmma"
    # alpha / beta through the same epilogue
    C0 = bf16_bits(rng, N * L * n_out) if bf else bits(rand(rng, N * L * n_out, np.float16))
    mk = (lambda x: bf16_dev(x)) if bf else (lambda x: torch.from_numpy(x.view(np.int16)).cuda().view(torch.float16))
    C3, C4 = mk(C0.copy()), mk(C0.copy())
    gpu.spmma(blob, dB, C3, L, n_out, K, N, 0, alpha=0.5, beta=-1.5)
    gpu.conv_spmma_fused(dX, dB, C4, N, Cin, H, W, kh, kw, s_, p_, d_, n_out, alpha=0.5, beta=-1.5)
    assert torch.equal(C3.view(torch.int16), C4.view(torch.int16))
    # the oracle, on the first image
    if not bf:
        A = orc.im2col(X[:Cin * H * W], 1, Cin, H, W, kh, kw, s_, p_, d_)
        ob = orc.compress24(A, L, K, K)
        Cref = np.zeros(L * n_out, dtype=np.uint16)
        orc.spmma(ob, Bw, Cref, L, n_out, K)
        P = np.abs(orc.decompress24(ob, L, K, K, np.uint16).view(np.float16).astype(np.float64)).reshape(L, K)
        scale = (P @ np.abs(Bw.view(np.float16).astype(np.float64)).reshape(K, n_out)).reshape(-1)
        check_close(host(C2[:L * n_out]), Cref.view(np.float16), scale, FP16_TOL, f"conv implicit {case}", K)


def test_conv_spmma_routes_agree_bf16(gpu):
    """the routed entry in bfloat16 on the geometry that takes the blob route: same bits as the pair"""
    import torch
    N, Cin, H, W, n_out = 2, 512, 14, 14, 256
    L, K = H * W, Cin * 9
    rng = np.random.default_rng(9)
    dX, dB = bf16_dev(bf16_bits(rng, N * Cin * H * W)), bf16_dev(bf16_bits(rng, K * n_out))
    blob = torch.empty(gpu.compress24_size(L, K, 2, N), dtype=torch.uint8, device="cuda")
    gpu.im2col(dX, N, Cin, H, W, 3, 3, 1, 1, 1, blob, compress=True)
    want = torch.zeros(N * L * n_out, dtype=torch.bfloat16, device="cuda")
    gpu.spmma(blob, dB, want, L, n_out, K, N, 0)
    ws = torch.empty(gpu.conv_spmma_workspace(N, Cin, H, W, 3, 3, 1, 1, 1), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    got = torch.full_like(want, 3.0)
    gpu.conv_spmma(dX, dB, got, N, Cin, H, W, 3, 3, 1, 1, 1, n_out, workspace=ws)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("geom", [(2, 512, 14, 14, 512), (2, 256, 16, 16, 64), (2, 64, 28, 28, 64), (1, 3, 16, 16, 64, 7)], ids=lambda g_: "x".join(map(str, g_)))
def test_conv_spmma_routes_agree(gpu, geom):
    """sm_conv_spmma_f16: the faster route per layer -- the implicit-GEMM kernel, or (out_h * out_w <= 256 with K >= 2048)
    sm_im2col_compress24 into the workspace + sm_spmma -- gives the C of the pair bit for bit whichever route runs, with and
    without a workspace; a geometry the implicit kernel declines (7 x 7 window on 3 channels: K = 147) runs the pair when a
    workspace is given and is declined without one."""
    import torch
    N, Cin, H, W, n_out = geom[:5]
    kh = kw = geom[5] if len(geom) > 5 else 3
    pad = kh // 2
    OH, OW = gpu.conv_out_size(H, kh, 1, pad, 1), gpu.conv_out_size(W, kw, 1, pad, 1)
    L, K = OH * OW, Cin * kh * kw
    rng = np.random.default_rng(Cin + H)
    dX = to_dev(rand(rng, N * Cin * H * W, np.float16))
    dB = to_dev(rand(rng, K * n_out, np.float16))
    blob = torch.empty(gpu.compress24_size(L, K, 2, N), dtype=torch.uint8, device="cuda")
    gpu.im2col(dX, N, Cin, H, W, kh, kw, 1, pad, 1, blob, compress=True)
    want = torch.zeros(N * L * n_out, dtype=torch.float16, device="cuda")
    gpu.spmma(blob, dB, want, L, n_out, K, N, 0)
    need = gpu.conv_spmma_workspace(N, Cin, H, W, kh, kw, 1, pad, 1)
    # the blob's size where the rule prefers the pair AND where the implicit kernel cannot run the geometry, else 0
    assert (need > 0) == ((L <= 256 and K >= 2048) or K % 64 != 0)
    if need:
        assert need == gpu.compress24_size(L, K, 2, N)
    ws = torch.empty(need or gpu.compress24_size(L, K, 2, N), dtype=torch.uint8, device="cuda")
    got = torch.full_like(want, 3.0)
    gpu.conv_spmma(dX, dB, got, N, Cin, H, W, kh, kw, 1, pad, 1, n_out, workspace=ws)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    got.fill_(5.0)
    if K % 64 == 0:
        gpu.conv_spmma(dX, dB, got, N, Cin, H, W, kh, kw, 1, pad, 1, n_out)          # no workspace: the implicit kernel
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    else:
        with pytest.raises(gpu.SparsifymeError, match="status 2"):
            gpu.conv_spmma(dX, dB, got, N, Cin, H, W, kh, kw, 1, pad, 1, n_out)


def test_conv_spmma_fused_rejects_what_it_cannot_take(gpu):
    import torch
    x = torch.zeros(4096, dtype=torch.float16, device="cuda")
    L_ = gpu.lib()
    args = lambda N, C, H, W, kh, kw, s_, p_, d_, n: (x.data_ptr(), x.data_ptr(), x.data_ptr(), N, C, H, W, kh, kw, s_, p_, d_, n, 1.0, 0.0, None)
    assert L_.sm_conv_spmma_fused_f16(*args(1, 3, 8, 8, 7, 7, 2, 3, 1, 64)) == 2      # K = 147: not whole stages (NOT_SUPPORTED)
    assert L_.sm_conv_spmma_fused_f16(*args(1, 64, 8, 9, 3, 3, 1, 1, 1, 64)) == 2      # odd W
    assert L_.sm_conv_spmma_fused_f16(*args(1, 64, 4, 4, 5, 5, 1, 0, 1, 64)) == 1      # window larger than the input (INVALID_VALUE)
    assert L_.sm_conv_spmma_fused_f16(*args(1, 64, 8, 8, 3, 3, 0, 1, 1, 64)) == 1      # zero stride


def test_im2col_rejects_bad_windows(gpu):
    import torch
    x = torch.zeros(64, dtype=torch.float16, device="cuda")
    L_ = gpu.lib()
    assert L_.sm_im2col_f16(x.data_ptr(), 1, 1, 4, 4, 5, 5, 1, 0, 1, x.data_ptr(), None) == 1      # window larger than the image
    assert L_.sm_im2col_f16(x.data_ptr(), 1, 1, 4, 4, 3, 3, 0, 0, 1, x.data_ptr(), None) == 1      # zero stride
    assert L_.sm_im2col_f16(None, 1, 1, 4, 4, 3, 3, 1, 0, 1, x.data_ptr(), None) == 1


def test_two_host_threads_two_streams(gpu):
    """Concurrent callers: two host threads, each on its own HIP stream, run the fused and the staged 2:4 matmuls (kernels
    that opt in to > 64 KiB of LDS on first use -- the opt-in is per device and must tolerate a race on the first call)
    on different problems at the same time; every result must equal the single-threaded one bit for bit."""
    import threading
    import torch
    shapes = [(196, 512, 1024, 4), (784, 1024, 256, 2), (300, 520, 576, 2), (3136, 128, 1152, 1)]
    probs = []
    g = torch.Generator(device="cuda").manual_seed(11)
    for (m, n, k, b) in shapes:
        A = (torch.rand(b * m * k, generator=g, device="cuda") - 0.5).half()
        B = (torch.rand(k * n, generator=g, device="cuda") - 0.5).half()
        blob = torch.empty(gpu.compress24_size(m, k, 2, b), dtype=torch.uint8, device="cuda")
        gpu.compress24(A, m, k, k, b, m * k, blob)
        ref = torch.empty(b * m * n, dtype=torch.float16, device="cuda")
        gpu.spmma(blob, B, ref, m, n, k, b, 0)
        probs.append((m, n, k, b, A, B, blob, ref))
    torch.cuda.synchronize()
    errors = []

    def worker(idx):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for rep in range(6):
                    for j, (m, n, k, b, A, B, blob, ref) in enumerate(probs):
                        if (j + idx) % 2:
                            continue
                        out = torch.full_like(ref, 3.0)
                        if rep % 2:
                            gpu.spmma(blob, B, out, m, n, k, b, 0)
                        else:
                            gpu.spmma_fused(A, B, out, m, n, k, batch=b)
                        st.synchronize()
                        if not torch.equal(out.view(torch.int16), ref.view(torch.int16)):
                            errors.append((idx, rep, j))
        except Exception as e:  # noqa: BLE001 -- reported by the assert below
            errors.append((idx, repr(e)))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_entry_points_are_graph_capturable(gpu):
    """C-ABI calls only enqueue on the given stream (no allocation, no synchronisation), so a
    whole pipeline can be captured into a hipGraph and replayed; the replay must reproduce the eager results."""
    import torch
    m, n, k, b = 196, 64, 128, 2
    g = torch.Generator(device="cuda").manual_seed(1)
    A0 = torch.rand(b * m * k, generator=g, device="cuda").half()
    B = torch.rand(k * n, generator=g, device="cuda").half()
    A8 = torch.randint(-128, 128, (b * m * k,), generator=g, device="cuda", dtype=torch.int8)
    B8 = torch.randint(-128, 128, (n * k,), generator=g, device="cuda", dtype=torch.int8)
    X = torch.rand(2 * 8 * 12 * 12, generator=g, device="cuda").half()
    bufs = dict(A=A0.clone(), P=torch.empty_like(A0), valid=torch.zeros(1, dtype=torch.int32, device="cuda"),
                blob=torch.empty(gpu.compress24_size(m, k, 2, b), dtype=torch.uint8, device="cuda"),
                back=torch.empty_like(A0), C=torch.empty(b * m * n, dtype=torch.float16, device="cuda"),
                Cf=torch.empty(b * m * n, dtype=torch.float16, device="cuda"), Cd=torch.empty(b * m * n, dtype=torch.float16, device="cuda"),
                blob8=torch.empty(gpu.compress24_size(m, k, 1, b), dtype=torch.uint8, device="cuda"),
                C8=torch.empty(b * m * n, dtype=torch.int32, device="cuda"), Q8=torch.empty(b * m * n, dtype=torch.int8, device="cuda"),
                im=torch.empty(2 * 144 * 72, dtype=torch.float16, device="cuda"),
                mask=torch.empty(m * k, dtype=torch.int64, device="cuda"), W=A0[: m * k].clone())

    def pipeline(o):
        gpu.prune24(o["A"], o["P"], b * m, k, k, gpu.PRUNE_TILE)
        gpu.prune24_check(o["P"], b * m, k, k, o["valid"])
        gpu.compress24(o["P"], m, k, k, b, m * k, o["blob"])
        gpu.decompress24(o["blob"], m, k, k, b, m * k, o["back"])
        gpu.spmma(o["blob"], B, o["C"], m, n, k, b, 0)
        gpu.spmma_fused(o["P"], B, o["Cf"], m, n, k, batch=b)
        gpu.gemm_rowmajor(o["P"], B, o["Cd"], m, n, k, batch=b)
        gpu.compress24(A8, m, k, k, b, m * k, o["blob8"])
        gpu.spmma_i8(o["blob8"], B8, o["C8"], m, n, k, b, 0)
        gpu.spmma_fused_i8(A8, B8, o["Q8"], m, n, k, batch=b, scale=2.0 ** -9)
        gpu.im2col(X, 2, 8, 12, 12, 3, 3, 1, 1, 1, o["im"])
        gpu.sparsify(o["W"], o["mask"], m, k, 0.5)

    eager = {kk: v.clone() for kk, v in bufs.items()}
    pipeline(eager)
    torch.cuda.synchronize()
    graphed = {kk: v.clone() for kk, v in bufs.items()}
    pipeline(graphed)          # first call outside capture (lazy function attributes)
    torch.cuda.synchronize()
    for kk in ("P", "valid", "blob", "back", "C", "Cf", "Cd", "blob8", "C8", "Q8", "im", "mask"):
        graphed[kk].fill_(0) if graphed[kk].dtype != torch.float16 else graphed[kk].zero_()
    graphed["W"].copy_(bufs["W"])
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=torch.cuda.Stream()):
        pipeline(graphed)
    gr.replay()
    torch.cuda.synchronize()
    for kk in eager:
        assert torch.equal(eager[kk].view(torch.uint8), graphed[kk].view(torch.uint8)), f"graph replay differs from eager in {kk}"


def test_fused_rejects_what_it_cannot_take(gpu):
    import torch
    A = torch.zeros(16 * 147, dtype=torch.float16, device="cuda")
    B = torch.zeros(147 * 64, dtype=torch.float16, device="cuda")
    C = torch.zeros(16 * 64, dtype=torch.float16, device="cuda")
    gpu.spmma_fused(A, B, C, 16, 64, 147)       # k % 64 != 0, n <= 128, contiguous rows: the span form takes it (round 3)
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fused(A, B, C, 16, 64, 147, lda=152)   # padded rows: caller must use compress + spmma
    B2 = torch.zeros(147 * 256, dtype=torch.float16, device="cuda")
    C2 = torch.zeros(16 * 256, dtype=torch.float16, device="cuda")
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fused(A, B2, C2, 16, 256, 147)         # k % 64 != 0 with n > 128


# ---------------------------------------------------------------------------------------------
# empty problems: every entry point is a successful no-op for a zero extent, and a zero-length k leaves
# C = beta * C (the sum over k is empty) -- the reference's vendor calls accept these sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", ["m", "n", "batch"])
def test_empty_extents_are_noops(gpu, zero):
    import torch
    m, n, k, b = 64, 64, 128, 2
    dims = {"m": m, "n": n, "batch": b}
    dims[zero] = 0
    m, n, b = dims["m"], dims["n"], dims["batch"]
    sentinel = 3.25
    for tdt in (torch.float16, torch.bfloat16, torch.float32):
        A = torch.ones(max(1, b * m * k), dtype=tdt, device="cuda")
        B = torch.ones(max(1, b * k * n), dtype=tdt, device="cuda")
        C = torch.full((max(1, 2 * 64 * 64),), sentinel, dtype=tdt, device="cuda")
        gpu.gemm_rowmajor(A, B, C, m, n, k, batch=b, strideA=m * k, strideB=k * n, strideC=m * n)
        gpu.spmma_fused(A, B, C, m, n, k, batch=b, strideA=m * k, strideB=k * n, strideC=m * n)
        esz = A.element_size()
        blob = torch.zeros(max(16, gpu.compress24_size(m, k, esz, b)), dtype=torch.uint8, device="cuda")
        if zero != "n":
            gpu.compress24(A, m, k, k, b, m * k, blob)
            gpu.decompress24(blob, m, k, k, b, m * k, A)
        gpu.spmma(blob, B, C, m, n, k, batch=b, strideB=k * n, strideC=m * n)
        assert bool((C == sentinel).all()), (zero, tdt)
    # prune / check / one-pass / transpose on an empty matrix
    A16 = torch.ones(16, dtype=torch.float16, device="cuda")
    O16 = torch.full((16,), sentinel, dtype=torch.float16, device="cuda")
    valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    blob = torch.zeros(64, dtype=torch.uint8, device="cuda")
    gpu.prune24(A16, O16, 0, 64, 64, gpu.PRUNE_TILE)
    gpu.prune24(A16, O16, 0, 64, 64, gpu.PRUNE_STRIP)
    gpu.prune24_compress24(A16, O16, 0, 64, 64, 1, 0, blob, valid, gpu.PRUNE_TILE)
    gpu.transpose(A16, O16, 0, 8)
    gpu.transpose(A16, O16, 8, 0)
    assert bool((O16 == sentinel).all())
    # an empty matrix is trivially 2:4: both the one-pass call above and the check write "valid" (0) over the stale flag
    assert int(host(valid)[0]) == 0
    valid.fill_(7)
    gpu.prune24_check(A16, 0, 64, 64, valid)
    assert int(host(valid)[0]) == 0


@pytest.mark.parametrize("tname", ["f16", "bf16", "f32"])
def test_zero_length_k_scales_c_by_beta(gpu, tname):
    import torch
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[tname]
    m, n, b = 96, 72, 2
    A = torch.ones(8, dtype=tdt, device="cuda")
    B = torch.ones(8, dtype=tdt, device="cuda")
    blob = torch.zeros(16, dtype=torch.uint8, device="cuda")
    C0 = torch.arange(b * m * n, device="cuda").remainder(17).to(tdt)
    for call in ("gemm", "spmma", "fused"):
        for beta in (0.0, 0.5):
            C = C0.clone()
            if call == "gemm":
                gpu.gemm_rowmajor(A, B, C, m, n, 0, lda=8, batch=b, strideA=0, strideB=0, strideC=m * n, alpha=2.0, beta=beta)
            elif call == "spmma":
                gpu.spmma(blob, B, C, m, n, 0, batch=b, strideB=0, strideC=m * n, alpha=2.0, beta=beta)
            else:
                gpu.spmma_fused(A, B, C, m, n, 0, lda=8, batch=b, strideA=0, strideB=0, strideC=m * n, alpha=2.0, beta=beta)
            want = (C0.float() * beta).to(tdt)
            assert torch.equal(C, want), (call, beta, tname)


def test_spmm_coo_packed_dense_rows_and_bad_columns(gpu, orc):
    """Sixteen half-dense rows among sparse ones (row lengths far from the pad unit), and column indices outside [0, cols),
    which are skipped as in the CSR kernels."""
    import torch
    m, k, n, batches = 48, 256, 40, 2
    rng = np.random.default_rng(99)
    dense = rng.random((m, k)) < 0.1
    dense[0:16, 0:128] = True
    r, c = np.nonzero(dense)
    r, c = r.astype(np.int32), c.astype(np.int32)
    v = rng.uniform(-1, 1, r.size).astype(np.float32)
    B = rng.uniform(-1, 1, batches * k * n).astype(np.float32)
    C0 = rng.uniform(-1, 1, batches * m * n).astype(np.float32)
    want = C0.copy()
    orc.spmm_coo(m, k, r.size, n, batches, r, c, v, B, want, 0.5, 2.0)
    dC, dr, dc, dv, dB = to_dev(C0.copy()), to_dev(r), to_dev(c), to_dev(v), to_dev(B)
    ws = _coo_call(gpu, "packed", m, k, r.size, n, batches, dr, dc, dv, dB, dC, 0.5, 2.0)
    assert int(host(ws[:4].view(torch.int32))[0]) == 4
    assert np.allclose(host(dC), want, rtol=2e-5, atol=2e-5)
    # a sparse problem with two out-of-range columns: skipped, the rest exact
    r2, c2, v2, rng = _coo_problem(m, k, 5, 0.08)
    c3 = c2.copy()
    c3[3] = k + 7
    c3[-2] = -1
    ok = (c3 >= 0) & (c3 < k)
    want = C0.copy()
    orc.spmm_coo(m, k, int(ok.sum()), n, batches, r2[ok].copy(), c3[ok].copy(), v2[ok].copy(), B, want, 1.0, 1.0)
    dC = to_dev(C0.copy())
    ws = _coo_call(gpu, "packed", m, k, r2.size, n, batches, to_dev(r2), to_dev(c3), to_dev(v2), dB, dC, 1.0, 1.0)
    assert int(host(ws[:4].view(torch.int32))[0]) == 4
    assert np.allclose(host(dC), want, rtol=2e-5, atol=2e-5)


def test_spmm_coo_packed_is_deterministic_and_graph_capturable(gpu):
    """Same input, same bits (a row's products are added in input order, chunk by chunk; no atomics on the sorted path), also
    when the whole call -- preprocessing included -- is replayed from a hipGraph."""
    import ctypes
    import torch
    m, k, n, batches = 784, 2304, 24, 2
    r, c, v, rng = _coo_problem(m, k, 4242)
    dr, dc, dv = to_dev(r), to_dev(c), to_dev(v)
    dB = torch.empty(batches * k * n, dtype=torch.float32, device="cuda")
    gpu.fill_uniform(dB, 17, -1.0, 1.0)
    nb = ctypes.c_size_t(0)
    assert gpu.lib().sm_spmm_coo_packed_workspace_size(m, r.size, ctypes.byref(nb)) == 0
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        dC = torch.zeros(batches * m * n, dtype=torch.float32, device="cuda")
        assert gpu.lib().sm_spmm_coo_f32_packed(m, k, r.size, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(),
                                                 dC.data_ptr(), 1.0, 0.0, ws.data_ptr(), nb.value, None) == 0
        outs.append(host(dC).copy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    dC = torch.zeros(batches * m * n, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        assert gpu.lib().sm_spmm_coo_f32_packed(m, k, r.size, n, batches, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dB.data_ptr(),
                                                 dC.data_ptr(), 1.0, 0.0, ws.data_ptr(), nb.value,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    g.replay()
    assert np.array_equal(bits(host(dC)), bits(outs[0]))


@pytest.mark.parametrize("entry", ["ws", "packed"])
def test_spmm_coo_without_non_zeros_scales_c_by_beta(gpu, entry):
    """nnz = 0: C = beta * C (beta = 0 must also clear a NaN); zero rows / vectors: a successful no-op."""
    import torch
    m, k, n, batches = 40, 64, 12, 2
    dr = torch.zeros(4, dtype=torch.int32, device="cuda")
    dv = torch.zeros(4, dtype=torch.float32, device="cuda")
    dB = torch.ones(batches * k * n, dtype=torch.float32, device="cuda")
    for beta in (0.0, -2.0):
        dC = torch.arange(batches * m * n, device="cuda").remainder(9).float()
        dC[3] = float("nan") if beta == 0.0 else 1.0
        want = torch.zeros_like(dC) if beta == 0.0 else dC * beta
        _coo_call(gpu, entry, m, k, 0, n, batches, dr, dr, dv, dB, dC, 1.0, beta)
        assert torch.equal(dC, want), (entry, beta)
    dC = torch.full((16,), 7.0, device="cuda")
    _coo_call(gpu, entry, 0, k, 0, n, batches, dr, dr, dv, dB, dC, 1.0, 0.0)
    _coo_call(gpu, entry, m, k, 0, 0, batches, dr, dr, dv, dB, dC, 1.0, 0.0)
    assert bool((dC == 7.0).all())
