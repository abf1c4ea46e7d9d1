"""Per-row fp8 quantisation of a 16-bit A on the device (quant_fp8.hip), dense and fused with the 2:4 compress, and the
weight operand's quantise + transpose.  The specification is restated here in numpy (ref_quant_rows / ref_quant_transpose):

    amax_i = max(max_j |a_ij| over the finite elements, 2^-100);  row_scale_i = amax_i / FMAX;  inv_i = FMAX / amax_i  (fp32)
    q_ij = float8(fp32(fp32(a_ij) * inv_i))  (round to nearest even);  NaN -> 0x7f, +-inf -> 0x7f (e4m3) / 0x7c | sign (e5m2)

and the device must match it byte for byte (Q, the blob) and bit for bit (row_scale).  The compress form is, by
construction, sm_compress24_fp8 of the quantised matrix, so the existing fp8 kernels and the CPU oracle on the fp16 image
are its references.  End to end the product is held against the fp64 product of the ORIGINAL 16-bit A on the kept
positions within the derived quantisation bound |a - row_scale q| <= R |a| + S row_scale plus the arithmetic bound of
tests/test_gpu_fp8.py."""
import os

import numpy as np
import pytest

from b8_testlib import FMAX, FMTS, ROUND, TINY, bytes_of, cast8, img16, nonfinite_bytes, ref_quant_rows, tdt, val64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = ["f16", "bf16"]
# |a - row_scale q| <= R |a| + S row_scale: half an ulp of the format's normals, half its smallest subnormal
QR = {"e4m3": 2.0 ** -4, "e5m2": 2.0 ** -3}
QS = {"e4m3": 2.0 ** -10, "e5m2": 2.0 ** -17}
# (rows, k, lda, ldq); k = 16448 = 32 x 512 + 64 lies beyond what a lane holds in registers (the re-reading form)
SHAPES = [(2, 64, 64, 64), (6, 128, 128, 128), (7, 100, 104, 100), (130, 192, 192, 192), (196, 512, 512, 512), (1568, 2304, 2304, 2304),
          (64, 4608, 4608, 4608), (33, 576, 584, 592), (34, 16448, 16448, 16448)]
KINDS = ["normal", "relu", "ties", "mixed"]


def sdt(s):
    import torch
    return {"f16": torch.float16, "bf16": torch.bfloat16}[s]


def bits16(t):
    import torch
    return t.view(torch.int16).numpy().view(np.uint16)


def f32_bits(t):
    import torch
    return t.view(torch.int32).cpu().numpy()


def ref_quant_transpose(x, inv_scale, f):
    """x: k x n float32 -> Bt bytes n x k, saturating."""
    fm = np.float32(FMAX[f])
    fin = np.isfinite(x)
    y = np.clip((np.where(fin, x, np.float32(0)) * np.float32(inv_scale)).astype(np.float32), -fm, fm)
    return np.ascontiguousarray(nonfinite_bytes(x, cast8(y, f), f).T)


def strip_keep(q):
    """STRIP keep mask of fp8 bytes (finite): the two largest bits & 0x7f per strip of 4, ties keep the lower k."""
    rows, k = q.shape
    key = ((q.reshape(rows, k // 4, 4) & 0x7F).astype(np.int32) << 2) | (3 - np.arange(4, dtype=np.int32))
    second = np.sort(key, axis=2)[:, :, 2:3]
    return (key >= second).reshape(rows, k)


def make_a(rng, rows, k, src, kind):
    """a 16-bit torch tensor rows x k (CPU)."""
    import torch
    x = rng.standard_normal((rows, k)).astype(np.float32)
    if kind == "relu":
        x = np.maximum(x, 0)
    elif kind == "ties":
        x = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 0.75, -0.75, 3.0], dtype=np.float32), (rows, k))
    elif kind == "mixed":
        for i in range(rows):
            c = i % 8
            if c == 0:
                x[i] = 0
            elif c == 1:
                x[i] = 0
                x[i, int(rng.integers(0, k))] = -2.5
            elif c == 2:
                x[i] *= 1e-6
            elif c == 3:
                x[i] = np.clip(x[i] * 1e4, -60000, 60000)
            elif c == 4:
                # fp16: subnormals (below 2^-14); bf16: small normals, magnitudes kept at 0 or above 2^-98
                x[i] = x[i] * (2.0 ** -17 if src == "f16" else 2.0 ** -90)
                if src == "bf16":
                    x[i][np.abs(x[i]) < 2.0 ** -98] = 0
            elif c == 5:
                x[i] = np.where(rng.random(k) < 0.9, 0, x[i])
    return torch.from_numpy(x).to(sdt(src))


def padded(t, ld, fill):
    """rows x ld copy of t (rows x k) with `fill` in the padding columns."""
    import torch
    rows, k = t.shape
    out = torch.full((rows, ld), fill, dtype=t.dtype)
    out[:, :k] = t
    return out


# ---------------------------------------------------------------------------------------------
# dense form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FMTS)
@pytest.mark.parametrize("src", SRCS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s_: "x".join(map(str, s_)))
def test_quantize_rows_fp8_matches_the_numpy_rule(gpu, f, src, shape):
    import torch
    rows, k, lda, ldq = shape
    rng = np.random.default_rng(rows * 7 + k + 3 * FMTS.index(f) + SRCS.index(src))
    for kind in KINDS:
        a = make_a(rng, rows, k, src, kind)
        wantQ, wantS = ref_quant_rows(a.float().numpy(), f)
        dA = padded(a, lda, float("nan")).cuda()       # a kernel that read the padding would see it in amax / as NaN bytes
        Q = torch.full((rows, ldq), 0x55, dtype=torch.uint8, device="cuda")
        rs = torch.full((rows,), -1.0, dtype=torch.float32, device="cuda")
        gpu.quantize_rows_fp8(dA, Q.view(tdt(f)), rs, rows, k, lda=lda, ldq=ldq)
        got = Q.cpu().numpy()
        assert np.array_equal(rs.cpu().numpy().view(np.uint32), wantS.view(np.uint32)), f"{src}->{f} {shape} {kind}: row_scale"
        assert np.array_equal(got[:, :k], wantQ), f"{src}->{f} {shape} {kind}: Q"
        assert (got[:, k:] == 0x55).all(), f"{src}->{f} {shape} {kind}: padding of Q written"
        if kind in ("normal", "relu"):   # the largest element of a non-zero row becomes the top finite byte
            assert ((got[:, :k] & 0x7F).max(axis=1) == (0x7E if f == "e4m3" else 0x7B)).all()


@pytest.mark.parametrize("f", FMTS)
@pytest.mark.parametrize("src", SRCS)
def test_quantize_rows_fp8_non_finite_policy(gpu, f, src):
    import torch
    rows, k = 6, 64
    nan, inf = float("nan"), float("inf")
    x = np.zeros((rows, k), dtype=np.float32)
    x[0, :8] = [1.0, -2.0, nan, inf, -inf, 4.0, -0.0, 0.5]       # amax = 4, not inf
    x[1, :] = nan                                                   # nothing finite: amax = 2^-100
    x[2, 5], x[2, 40] = inf, -3.0
    x[3, 63] = -inf                                                 # the rest zero: amax = 2^-100
    x[4, :4] = [-nan, 8.0, 8.0, -8.0]
    x[5, :] = np.linspace(-1, 1, k)                                 # a finite row next to them
    a = torch.from_numpy(x).to(sdt(src))
    a.view(torch.int16)[4, 0] = -1                                  # a negative NaN with a full payload (0xffff)
    xs = a.float().numpy()
    wantQ, wantS = ref_quant_rows(xs, f)
    assert wantS[0] == np.float32(4.0) / np.float32(FMAX[f]) and wantS[1] == np.float32(2.0 ** -100) / np.float32(FMAX[f])
    top = 0x7E if f == "e4m3" else 0x7B
    assert list(wantQ[0, 2:6]) == [0x7F, 0x7F if f == "e4m3" else 0x7C, 0x7F if f == "e4m3" else 0xFC, top]
    assert wantQ[4, 0] == 0x7F and list(wantQ[4, 1:4]) == [top, top, top | 0x80] and wantQ[0, 6] == 0x80
    Q = torch.empty((rows, k), dtype=torch.uint8, device="cuda")
    rs = torch.empty(rows, dtype=torch.float32, device="cuda")
    gpu.quantize_rows_fp8(a.cuda(), Q.view(tdt(f)), rs, rows, k)
    assert np.array_equal(Q.cpu().numpy(), wantQ)
    assert np.array_equal(rs.cpu().numpy().view(np.uint32), wantS.view(np.uint32))
    blob = torch.empty(gpu.compress24_size(rows, k, 1, 1), dtype=torch.uint8, device="cuda")
    want_blob = torch.empty_like(blob)
    rs2 = torch.empty_like(rs)
    gpu.quantize_compress24_fp8(a.cuda(), blob, rs2, rows, k, tdt(f))
    gpu.compress24_fp8(torch.from_numpy(wantQ).cuda().view(tdt(f)), rows, k, k, 1, rows * k, want_blob)
    assert torch.equal(blob, want_blob) and torch.equal(rs2, rs)


# ---------------------------------------------------------------------------------------------
# compress form
# ---------------------------------------------------------------------------------------------
def _sections(orc, blob, m, k, elt):
    kc, meta_off, _ = orc.compress24_layout(m, k, elt, 1)
    return blob[: m * kc // 2 * elt], blob[meta_off: meta_off + m * kc // 8]


@pytest.mark.parametrize("f", FMTS)
@pytest.mark.parametrize("src", SRCS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % 64 == 0], ids=lambda s_: "x".join(map(str, s_)))
def test_quantize_compress24_fp8_is_compress_of_the_quantised_matrix(gpu, orc, f, src, shape):
    import torch
    rows, k, lda, _ = shape
    rng = np.random.default_rng(rows * 11 + k + 5 * FMTS.index(f) + SRCS.index(src))
    size = gpu.compress24_size(rows, k, 1, 1)
    for kind in KINDS:
        a = make_a(rng, rows, k, src, kind)
        wantQ, wantS = ref_quant_rows(a.float().numpy(), f)
        dA = padded(a, lda, float("nan")).cuda()
        blob = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
        blob0 = torch.zeros(size, dtype=torch.uint8, device="cuda")
        rs = torch.full((rows,), -1.0, dtype=torch.float32, device="cuda")
        rs0 = torch.full((rows,), -1.0, dtype=torch.float32, device="cuda")
        gpu.quantize_compress24_fp8(dA, blob, rs, rows, k, tdt(f), lda=lda)
        gpu.quantize_compress24_fp8(dA, blob0, rs0, rows, k, tdt(f), lda=lda)
        tag = f"{src}->{f} {shape} {kind}"
        assert torch.equal(blob, blob0), f"{tag}: a 0xff pre-filled blob differs from a zeroed one (gap or tail not written)"
        assert np.array_equal(rs.cpu().numpy().view(np.uint32), wantS.view(np.uint32)) and torch.equal(rs, rs0), f"{tag}: row_scale"
        # sm_compress24_fp8 of the reference bytes
        dQ = torch.from_numpy(wantQ).cuda().view(tdt(f))
        want = torch.full((size,), 0xAA, dtype=torch.uint8, device="cuda")
        gpu.compress24_fp8(dQ, rows, k, k, 1, rows * k, want)
        got = blob.cpu().numpy()
        assert np.array_equal(got, want.cpu().numpy()), f"{tag}: blob vs sm_compress24_fp8 of the reference bytes"
        # the oracle's compress of their fp16 image
        im = img16(wantQ.reshape(-1), f)
        v16, meta16 = _sections(orc, orc.compress24(im, rows, k, k, 1), rows, k, 2)
        v8, meta8 = _sections(orc, got, rows, k, 1)
        assert np.array_equal(meta8, meta16), f"{tag}: strip codes differ from the fp16 blob of the image"
        assert np.array_equal(img16(v8, f), v16.view(np.uint16)), f"{tag}: kept values differ from the fp16 blob's"
        # the inverse is the STRIP-pruned reference Q, a valid 2:4 operand
        back = torch.full((rows * k,), 0x55, dtype=torch.uint8, device="cuda").view(tdt(f))
        gpu.decompress24_fp8(blob, rows, k, k, 1, rows * k, back)
        pruned = torch.empty_like(dQ)
        gpu.prune24_fp8(dQ, pruned, rows, k, k, gpu.PRUNE_STRIP)
        assert torch.equal(back.view(torch.uint8), pruned.view(torch.uint8).reshape(-1)), f"{tag}: decompress != prune STRIP of the reference Q"
        valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        gpu.prune24_check_fp8(back, rows, k, k, valid)
        assert int(valid.item()) == 0, f"{tag}: decompressed operand is not 2:4"


# ---------------------------------------------------------------------------------------------
# end to end at full size
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12544, 64, 64), (3136, 128, 1152), (784, 256, 2304), (196, 512, 4608)], ids=lambda s_: "x".join(map(str, s_)))
def test_quantize_compress_spmma_fp8_resnet50_b32(gpu, shape):
    """b = 32 stacked as one tall fp16 A, e4m3, shared B, bf16 C.  One pass == staged in every byte (blob, row_scale, C); on sampled
    rows Q / row_scale equal the numpy rule and C lies within the quantisation + arithmetic bound of the fp64 product of the original A
    on the kept positions with the dequantised B."""
    import torch
    m, n, k = shape
    f, out, batch = "e4m3", "bf16", 32
    assert (m, n, k, batch) in _resnet50_shapes()
    rows = batch * m
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    A = torch.randn(rows * k, generator=g, device="cuda").to(torch.float16).view(rows, k)
    A *= (torch.rand(rows, 1, generator=g, device="cuda") * 8 + 0.01).to(torch.float16)      # rows of different scales
    B = (torch.randn(k * n, generator=g, device="cuda") * 0.05).to(torch.float16).view(k, n)
    inv_b = float(np.float32(FMAX[f]) / np.float32(B.abs().max().item()))
    alpha = float(np.float32(1.0) / np.float32(inv_b))
    Bt = torch.empty(n * k, dtype=tdt(f), device="cuda")
    gpu.quantize_transpose_fp8(B, Bt, k, n, inv_b)
    size = gpu.compress24_size(rows, k, 1, 1)
    # one pass
    blob1 = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    rs1 = torch.empty(rows, dtype=torch.float32, device="cuda")
    gpu.quantize_compress24_fp8(A, blob1, rs1, rows, k, tdt(f))
    C1 = torch.empty(rows * n, dtype=torch.bfloat16, device="cuda")
    gpu.spmma_fp8(blob1, Bt, C1, rows, n, k, 1, 0, alpha=alpha, row_scale=rs1, a_dtype=tdt(f))
    # staged
    Q = torch.empty(rows * k, dtype=tdt(f), device="cuda")
    rs2 = torch.empty(rows, dtype=torch.float32, device="cuda")
    gpu.quantize_rows_fp8(A, Q, rs2, rows, k)
    blob2 = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
    gpu.compress24_fp8(Q, rows, k, k, 1, rows * k, blob2)
    C2 = torch.empty(rows * n, dtype=torch.bfloat16, device="cuda")
    gpu.spmma_fp8(blob2, Bt, C2, rows, n, k, 1, 0, alpha=alpha, row_scale=rs2, a_dtype=tdt(f))
    torch.cuda.synchronize()
    assert torch.equal(blob1, blob2), f"{shape}: one-pass blob != staged blob"
    assert torch.equal(rs1.view(torch.int32), rs2.view(torch.int32)), f"{shape}: row_scale"
    assert torch.equal(C1.view(torch.int16), C2.view(torch.int16)), f"{shape}: C"
    # sampled rows: first and last row block included
    rng = np.random.default_rng(k)
    pick = np.unique(np.concatenate([rng.integers(0, rows, 256), np.arange(16), np.arange(rows - 16, rows)]))
    ri = torch.from_numpy(pick).cuda()
    a = A[ri].float().cpu().numpy()
    wantQ, wantS = ref_quant_rows(a, f)
    assert np.array_equal(Q.view(torch.uint8).view(rows, k)[ri].cpu().numpy(), wantQ), f"{shape}: Q of sampled rows"
    assert np.array_equal(rs1[ri].cpu().numpy().view(np.uint32), wantS.view(np.uint32)), f"{shape}: row_scale of sampled rows"
    assert np.array_equal(bytes_of(Bt).reshape(n, k), ref_quant_transpose(B.float().cpu().numpy(), inv_b, f)), f"{shape}: Bt"
    keep = strip_keep(wantQ)
    bdq = np.float64(np.float32(alpha)) * val64(bytes_of(Bt), f).reshape(n, k)          # dequantised B, [n][k]
    a64 = np.where(keep, a.astype(np.float64), 0.0)
    s64 = wantS.astype(np.float64)[:, None]
    sq = np.where(keep, s64 * val64(wantQ.reshape(-1), f).reshape(wantQ.shape), 0.0)    # what the kernel multiplies, exactly
    ref = a64 @ bdq.T
    qbound = (np.where(keep, QR[f] * np.abs(a64) + QS[f] * s64, 0.0)) @ np.abs(bdq).T
    exact_q = sq @ bdq.T
    abound = ROUND[out] * np.abs(exact_q) + (2.0 * k + 4.0) * 2.0 ** -24 * (np.abs(sq) @ np.abs(bdq).T) + TINY[out]
    # the reference satisfies the per-element part on the CPU
    assert (np.abs(a64 - sq) <= np.where(keep, QR[f] * np.abs(a64) + QS[f] * s64, 0.0)).all()
    got = C1.view(rows, n)[ri].float().cpu().numpy().astype(np.float64)
    ratio = float((np.abs(got - ref) / (qbound + abound)).max())
    print(f"{shape}: max err / bound {ratio:.3f}; max |C - ref| / max |ref| {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
    assert np.isfinite(got).all() and ratio <= 1.0, f"{shape}: err / bound {ratio:.3f}"


def _resnet50_shapes():
    import csv
    with open(os.path.join(ROOT, "datasets", "resnet50.csv"), newline="") as fh:
        return set(tuple(int(x) for x in r[:4]) for r in list(csv.reader(fh))[1:] if r)


# ---------------------------------------------------------------------------------------------
# the weight operand
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FMTS)
@pytest.mark.parametrize("src", SRCS)
@pytest.mark.parametrize("shape", [(64, 8, 8), (147, 64, 64), (2304, 256, 256), (100, 33, 40)], ids=lambda s_: "x".join(map(str, s_)))
def test_quantize_transpose_fp8_matches_the_numpy_rule(gpu, f, src, shape):
    import torch
    k, n, ldb = shape
    rng = np.random.default_rng(k + 3 * n + FMTS.index(f) + 2 * SRCS.index(src))
    x = rng.standard_normal((k, n)).astype(np.float32)
    x[rng.random((k, n)) < 0.02] = np.float32("nan")
    x[rng.random((k, n)) < 0.02] = np.float32("inf")
    x[rng.random((k, n)) < 0.02] = -np.float32("inf")
    x[0, 0] = -0.0
    b = torch.from_numpy(x).to(sdt(src))
    for inv in (1.0, FMAX[f] / 1.5, 3.0e-3):        # the middle one saturates every |b| > 1.5
        want = ref_quant_transpose(b.float().numpy(), inv, f)
        if inv > 1.0:
            assert ((want & 0x7F) == (0x7E if f == "e4m3" else 0x7B)).sum() > k * n // 20
        Bt = torch.full((n * k + 3,), 0x55, dtype=torch.uint8, device="cuda")
        gpu.quantize_transpose_fp8(padded(b, ldb, float("nan")).cuda(), Bt[: n * k].view(tdt(f)), k, n, inv, ldb=ldb)
        got = Bt.cpu().numpy()
        assert np.array_equal(got[: n * k].reshape(n, k), want), f"{src}->{f} {shape} inv_scale {inv}"
        assert (got[n * k:] == 0x55).all()


# ---------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------
def test_quantize_entry_points_graph_capture_replays(gpu):
    import torch
    rows, n, k = 392, 96, 576
    g = torch.Generator(device="cuda").manual_seed(11)
    A = torch.randn(rows * k, generator=g, device="cuda").to(torch.bfloat16)
    B = torch.randn(k * n, generator=g, device="cuda").to(torch.bfloat16)
    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    Q = torch.empty(rows * k, dtype=e5, device="cuda")
    rsq = torch.empty(rows, dtype=torch.float32, device="cuda")
    blob = torch.empty(gpu.compress24_size(rows, k, 1, 1), dtype=torch.uint8, device="cuda")
    rsb = torch.empty(rows, dtype=torch.float32, device="cuda")
    Bt = torch.empty(n * k, dtype=e4, device="cuda")
    outs = (Q, rsq, blob, rsb, Bt)

    def step():
        gpu.quantize_rows_fp8(A, Q, rsq, rows, k)
        gpu.quantize_compress24_fp8(A, blob, rsb, rows, k, e4)
        gpu.quantize_transpose_fp8(B, Bt, k, n, 100.0)
    step()
    torch.cuda.synchronize()
    want = [t.view(torch.uint8).clone() for t in outs]
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for _ in range(2):
        for t in outs:
            t.view(torch.uint8).fill_(0x33)
        graph.replay()
        torch.cuda.synchronize()
        for name, t, w in zip(("Q", "row_scale of Q", "blob", "row_scale of the blob", "Bt"), outs, want):
            got = t.view(torch.uint8)
            d = (got != w).nonzero().flatten()
            assert d.numel() == 0, (f"{name}: {d.numel()} of {w.numel()} bytes differ after a replay, first at {d[:6].tolist()}: "
                                    f"{got[d[:6]].tolist()} for {w[d[:6]].tolist()}")
