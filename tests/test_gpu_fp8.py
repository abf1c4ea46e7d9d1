"""The OCP fp8 (e4m3 / e5m2) 2:4 path on the device (spmma_fp8.hip).  The rules are the fp16 rules on the exact fp16 image
of the bytes (torch's .to(float16)), so the CPU oracle and the GPU fp16 kernels on that image are the references: prune and
compress bit for bit, the matmul exactly on operands whose every fp32 partial sum is exact and otherwise within the
arithmetic bound (one rounding of the output type plus fp32 accumulation), the fused form bit for bit against the staged
sequence."""
import os
import subprocess

import numpy as np
import pytest

from b8_testlib import FMTS, OUTS, PAIRS, ROUND, TINY, bytes_of, dev8, finite_bytes, img16, make_bytes, map_back, odt, tdt, val64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------
# prune / check
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FMTS)
@pytest.mark.parametrize("shape", [(4, 4), (7, 10), (33, 17), (64, 128), (130, 147), (196, 512)])
def test_prune24_fp8_is_the_fp16_rule_on_the_image(gpu, orc, f, shape):
    import torch
    m, k = shape
    rng = np.random.default_rng(m * 31 + k + (7 if f == "e5m2" else 0))
    for kind in ("rand", "ties", "special"):
        a = make_bytes(rng, m * k, f, kind)
        im = img16(a, f)
        dA = dev8(a, f)
        d16 = torch.from_numpy(im.view(np.int16)).cuda().view(torch.float16)
        for alg in (gpu.PRUNE_STRIP, gpu.PRUNE_TILE):
            want = map_back(orc.prune24(im, m, k, k, alg), im, a)
            out = torch.empty_like(dA)
            gpu.prune24_fp8(dA, out, m, k, k, alg)
            assert np.array_equal(bytes_of(out), want), f"prune24_fp8 {f} {shape} {kind} alg {alg} vs oracle on the image"
            o16 = torch.empty_like(d16)
            gpu.prune24(d16, o16, m, k, k, alg)
            got16 = o16.view(torch.int16).cpu().numpy().view(np.uint16)
            assert np.array_equal(map_back(got16, im, a), want), f"prune24_f16 on the image {f} {shape} {kind} alg {alg}"
            inplace = dA.clone()
            gpu.prune24_fp8(inplace, inplace, m, k, k, alg)
            assert np.array_equal(bytes_of(inplace), want), f"prune24_fp8 in place {f} {shape} {kind} alg {alg}"
            valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
            gpu.prune24_check_fp8(out, m, k, k, valid)
            assert int(valid.item()) == 0


def test_prune24_fp8_e5m2_nan_payloads_key_as_their_image(gpu, orc):
    """0x7d (a signalling NaN) becomes 0x7f00 in fp16 and so outranks 0x7e (0x7e00): the key follows the image."""
    import torch
    a = np.array([0x7d, 0x7e, 0x01, 0x00, 0x7e, 0x00, 0x7f, 0x7d, 0x7c, 0x7e, 0xfd, 0x00, 0x80, 0x7c, 0x7e, 0xfc], dtype=np.uint8)
    im = img16(a, "e5m2")
    want = map_back(orc.prune24(im, 1, 16, 16, orc.STRIP), im, a)
    out = torch.empty(16, dtype=torch.float8_e5m2, device="cuda")
    gpu.prune24_fp8(dev8(a, "e5m2"), out, 1, 16, 16)
    assert np.array_equal(bytes_of(out), want)
    assert list(want[:4]) == [0x7d, 0x7e, 0, 0] and list(want[4:8]) == [0, 0, 0x7f, 0x7d] and list(want[12:]) == [0, 0x7c, 0x7e, 0]


@pytest.mark.parametrize("f", FMTS)
def test_prune24_check_fp8_zero_test(gpu, f):
    import torch
    valid = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    m, k = 3, 64
    base = np.zeros(m * k, dtype=np.uint8)
    base[::4] = 0x38
    base[1::4] = 0xb8
    gpu.prune24_check_fp8(dev8(base, f), m, k, k, valid)
    assert int(valid.item()) == 0
    three = base.copy()
    three[2 * k + 42] = 0x01  # strip 10 of row 2: three non-zeros
    gpu.prune24_check_fp8(dev8(three, f), m, k, k, valid)
    assert int(valid.item()) == 1
    negzero = base.copy()
    negzero[2::4] = 0x80  # -0 is zero: every strip still holds two non-zeros
    negzero[3::4] = 0x80
    gpu.prune24_check_fp8(dev8(negzero, f), m, k, k, valid)
    assert int(valid.item()) == 0
    nan = base.copy()
    nan[6] = 0x7f  # NaN is not zero
    gpu.prune24_check_fp8(dev8(nan, f), m, k, k, valid)
    assert int(valid.item()) == 1


# ---------------------------------------------------------------------------------------------
# compress / decompress
# ---------------------------------------------------------------------------------------------
def _sections(blob, m, k, elt, batch):
    kc, meta_off, _ = _layout(m, k, elt, batch)
    M = m * batch
    return blob[: M * kc // 2 * elt], blob[meta_off: meta_off + M * kc // 8]


def _layout(m, k, elt, batch):
    import __graft_entry__ as ge
    return ge.load_oracle().compress24_layout(m, k, elt, batch)


@pytest.mark.parametrize("f", FMTS)
@pytest.mark.parametrize("shape", [(2, 64, 1), (64, 128, 1), (130, 192, 3), (33, 147, 2), (196, 512, 2)])
def test_compress24_fp8_vs_oracle(gpu, orc, f, shape):
    import torch
    m, k, batch = shape
    rng = np.random.default_rng(m + 3 * k + batch)
    size = gpu.compress24_size(m, k, 1, batch)
    for kind in ("rand", "ties", "special", "nonneg"):
        a = rng.integers(0, 0x7d, m * k * batch).astype(np.uint8) if kind == "nonneg" else make_bytes(rng, m * k * batch, f, kind)
        dA = dev8(a, f)
        blob = torch.empty(size, dtype=torch.uint8, device="cuda")
        gpu.compress24_fp8(dA, m, k, k, batch, m * k, blob)
        got = blob.cpu().numpy()
        if kind == "nonneg":  # no sign bit, no NaN: the fp8 keys are the int8 ones
            assert np.array_equal(got, orc.compress24(a.view(np.int8), m, k, k, batch)), f"{f} {shape}: blob vs int8 oracle"
        im = img16(a, f)
        ob16 = orc.compress24(im, m, k, k, batch)
        v16, meta16 = _sections(ob16, m, k, 2, batch)
        v8, meta8 = _sections(got, m, k, 1, batch)
        assert np.array_equal(meta8, meta16), f"{f} {shape} {kind}: strip codes differ from the fp16 blob of the image"
        assert np.array_equal(img16(v8, f), v16.view(np.uint16)), f"{f} {shape} {kind}: kept values differ from the fp16 blob's"
        # the inverse: the STRIP-pruned operand
        back = torch.empty_like(dA)
        back.view(torch.uint8).fill_(0x55)
        gpu.decompress24_fp8(blob, m, k, k, batch, m * k, back)
        want = map_back(orc.prune24(im, m * batch, k, k, orc.STRIP), im, a)
        assert np.array_equal(bytes_of(back), want), f"{f} {shape} {kind}: decompress(compress(A)) != prune STRIP(A)"


@pytest.mark.parametrize("f", FMTS)
def test_compress24_fp8_negative_zero_groups(gpu, f):
    """Hand-written strips around 0x80 (-0, a zero here; -128 to the int8 rule)."""
    import torch
    groups = [([0x80, 0x80, 0x01, 0x00], (0, 2)), ([0x80, 0x00, 0x00, 0x05], (0, 3)), ([0x00, 0x80, 0x80, 0x80], (0, 1)),
              ([0x81, 0x80, 0x02, 0x80], (0, 2)), ([0x80, 0x7f, 0x80, 0xff], (1, 3)), ([0x00, 0x00, 0x80, 0x01], (0, 3))]
    m, k = 2, 64
    a = np.zeros(m * k, dtype=np.uint8)
    for q, (g, _) in enumerate(groups):
        a[4 * q: 4 * q + 4] = g
    blob = torch.empty(gpu.compress24_size(m, k, 1, 1), dtype=torch.uint8, device="cuda")
    gpu.compress24_fp8(dev8(a, f), m, k, k, 1, m * k, blob)
    vals, meta = _sections(blob.cpu().numpy(), m, k, 1, 1)
    for q, (g, (p0, p1)) in enumerate(groups):
        nib = (meta[q // 2] >> (4 * (q & 1))) & 0xF
        assert (nib & 3, nib >> 2) == (p0, p1), f"{f} group {q} {g}"
        assert (vals[2 * q], vals[2 * q + 1]) == (g[p0], g[p1]), f"{f} group {q} {g}"


# ---------------------------------------------------------------------------------------------
# matmul
# ---------------------------------------------------------------------------------------------
def _staged(gpu, a, Bt, fa, fb, m, n, k, batch, C, strideB=0, alpha=1.0, beta=0.0, row_scale=None):
    """prune STRIP -> compress -> spmma_fp8 on device operands; returns the pruned A (device)."""
    import torch
    dA = dev8(a, fa)
    gpu.prune24_fp8(dA, dA, m * batch, k, k, gpu.PRUNE_STRIP)
    blob = torch.empty(gpu.compress24_size(m, k, 1, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24_fp8(dA, m, k, k, batch, m * k, blob)
    gpu.spmma_fp8(blob, Bt, C, m, n, k, batch, strideB, alpha=alpha, beta=beta, row_scale=row_scale, a_dtype=tdt(fa))
    return dA


def _ref(pa, fa, bt, fb, m, n, k, batch, shared):
    """fp64 (A_b . B_b) per batch, and sum |a||b| (pa: pruned A bytes, bt: [n][k] bytes per batch)."""
    A = val64(pa, fa).reshape(batch, m, k)
    B = val64(bt, fb).reshape(1 if shared else batch, n, k)
    Bb = [B[0 if shared else i] for i in range(batch)]
    return (np.stack([A[i] @ Bb[i].T for i in range(batch)]), np.stack([np.abs(A[i]) @ np.abs(Bb[i]).T for i in range(batch)]))


def _host_out(C):
    import torch
    return C.float().cpu().numpy().astype(np.float64) if C.dtype != torch.float32 else C.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("shape", [(64, 64, 128, 1), (130, 72, 192, 2), (32, 48, 256, 3), (2, 8, 64, 1), (258, 200, 320, 2)])
def test_spmma_fp8_exact_operands(gpu, fa, fb, shape):
    """Values in {0, +-0.5, +-1, +-2, +-3, +-4}: every product and fp32 partial sum is exact, so the fp32 C must equal the
    fp64 product exactly -- which only holds if the instruction reads the operand lanes and index codes as the kernel feeds them."""
    import torch
    m, n, k, batch = shape
    rng = np.random.default_rng(m + n + k + 17 * batch + 3 * FMTS.index(fa) + FMTS.index(fb))
    vals = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0], dtype=np.float32)
    to8 = lambda x, f: torch.from_numpy(x).to(tdt(f)).view(torch.uint8).numpy().copy()
    a = to8(rng.choice(vals, m * k * batch), fa)
    for shared in (True, False):
        bt = to8(rng.choice(vals, n * k * (1 if shared else batch)), fb)
        C = torch.full((batch * m * n,), 9.0, dtype=torch.float32, device="cuda")
        pa = _staged(gpu, a, dev8(bt, fb), fa, fb, m, n, k, batch, C, 0 if shared else n * k)
        ref, _ = _ref(bytes_of(pa), fa, bt, fb, m, n, k, batch, shared)
        assert np.array_equal(_host_out(C).reshape(ref.shape), ref), f"{fa} x {fb} {shape} shared={shared}"


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("out", OUTS)
def test_spmma_fp8_random_operands_within_bound(gpu, fa, fb, out):
    import torch
    rng = np.random.default_rng(100 + 10 * FMTS.index(fa) + 3 * FMTS.index(fb) + OUTS.index(out))
    for (m, n, k, batch) in [(196, 256, 512, 2), (130, 72, 192, 3), (64, 520, 1024, 1)]:
        a = finite_bytes(rng, m * k * batch, fa)
        for shared, (alpha, beta, with_rs) in [(True, (1.0, 0.0, False)), (False, (0.75, 0.5, True)), (True, (-1.5, 1.0, True))]:
            bt = finite_bytes(rng, n * k * (1 if shared else batch), fb)
            C0 = torch.from_numpy(rng.uniform(-4, 4, batch * m * n).astype(np.float32)).to(odt(out)).cuda()
            C = C0.clone()
            rs = torch.from_numpy(rng.uniform(0.25, 2.0, m).astype(np.float32)).cuda() if with_rs else None
            pa = _staged(gpu, a, dev8(bt, fb), fa, fb, m, n, k, batch, C, 0 if shared else n * k, alpha, beta, rs)
            prod, absprod = _ref(bytes_of(pa), fa, bt, fb, m, n, k, batch, shared)
            s = alpha * (rs.cpu().numpy().astype(np.float64)[None, :, None] if with_rs else 1.0)
            c0 = _host_out(C0).reshape(prod.shape)
            ref = s * prod + beta * c0
            scale = np.abs(s) * absprod + abs(beta) * np.abs(c0)
            got = _host_out(C).reshape(prod.shape)
            # one rounding of the output type; fp32 accumulation (2k steps of 2^-24); the scale, beta and add roundings of fp32
            bound = ROUND[out] * np.abs(ref) + (2.0 * k + 4.0) * 2.0 ** -24 * scale + TINY[out]
            ratio = float((np.abs(got - ref) / bound).max())
            assert np.isfinite(got).all() and ratio <= 1.0, f"{fa} x {fb} -> {out} {(m, n, k, batch)} shared={shared}: err/bound {ratio:.3f}"


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_spmma_fp8_vs_spmma_f16_on_the_images(gpu, fa, fb):
    """the same products through sm_spmma_f16 on the exact fp16 images (B row-major k x n there)."""
    import torch
    m, n, k, batch = 196, 128, 576, 2
    rng = np.random.default_rng(7 + 2 * FMTS.index(fa) + FMTS.index(fb))
    a = finite_bytes(rng, m * k * batch, fa)
    bt = finite_bytes(rng, n * k, fb)
    C = torch.empty(batch * m * n, dtype=torch.float16, device="cuda")
    pa = _staged(gpu, a, dev8(bt, fb), fa, fb, m, n, k, batch, C)
    pa16 = dev8(bytes_of(pa), fa).to(torch.float16)
    blob16 = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
    gpu.compress24(pa16, m, k, k, batch, m * k, blob16)
    B16 = dev8(bt, fb).to(torch.float16).view(n, k).t().contiguous().view(-1)
    C16 = torch.empty_like(C)
    gpu.spmma(blob16, B16, C16, m, n, k, batch)
    prod, absprod = _ref(bytes_of(pa), fa, bt, fb, m, n, k, batch, True)
    bound = 2.0 * (ROUND["f16"] * np.abs(prod) + 2.0 * k * 2.0 ** -24 * absprod + TINY["f16"])
    diff = np.abs(_host_out(C) - _host_out(C16)).reshape(prod.shape)
    assert float((diff / bound).max()) <= 1.0, f"{fa} x {fb}: sm_spmma_fp8 vs sm_spmma_f16 on the images"


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("out", OUTS)
def test_spmma_fused_fp8_equals_staged(gpu, fa, fb, out):
    import torch
    rng = np.random.default_rng(300 + 10 * FMTS.index(fa) + 3 * FMTS.index(fb) + OUTS.index(out))
    for (m, n, k, batch, shared) in [(196, 256, 512, 2, True), (130, 72, 192, 3, False), (64, 40, 64, 1, True), (258, 200, 320, 2, True)]:
        a = make_bytes(rng, m * k * batch, fa, "rand")
        a[np.isin(a & 0x7F, [0x7F] if fa == "e4m3" else [0x7C, 0x7D, 0x7E, 0x7F])] = 0x38  # finite operands
        bt = finite_bytes(rng, n * k * (1 if shared else batch), fb)
        dB = dev8(bt, fb)
        rs = torch.from_numpy(rng.uniform(0.5, 2.0, m).astype(np.float32)).cuda()
        C0 = torch.from_numpy(rng.uniform(-1, 1, batch * m * n).astype(np.float32)).to(odt(out)).cuda()
        Cs, Cf = C0.clone(), C0.clone()
        sB = 0 if shared else n * k
        _staged(gpu, a, dB, fa, fb, m, n, k, batch, Cs, sB, 0.5, 0.25, rs)
        gpu.spmma_fused_fp8(dev8(a, fa), dB, Cf, m, n, k, batch=batch, strideB=sB, alpha=0.5, beta=0.25, row_scale=rs)
        torch.cuda.synchronize()
        assert torch.equal(Cs.view(torch.uint8) if out != "f32" else Cs.view(torch.int32),
                           Cf.view(torch.uint8) if out != "f32" else Cf.view(torch.int32)), f"{fa} x {fb} -> {out} {(m, n, k, batch)}"


def test_spmma_fp8_refuses_what_it_cannot_take(gpu):
    import torch
    blob = torch.zeros(gpu.compress24_size(16, 128, 1, 1), dtype=torch.uint8, device="cuda")
    B = torch.zeros(16 * 128, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fp8(blob, B, torch.zeros(256, dtype=torch.int32, device="cuda"), 16, 16, 128)   # C dtype
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fp8(blob, B, torch.zeros(256, device="cuda"), 16, 16, 100)                     # k % 64 != 0
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fp8(blob, B, torch.zeros(256, device="cuda"), 15, 16, 128)                     # odd m
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmma_fp8(blob, B.view(torch.int8), torch.zeros(256, device="cuda"), 16, 16, 128)    # B not fp8


# ---------------------------------------------------------------------------------------------
# full size, graph capture, driver
# ---------------------------------------------------------------------------------------------
def _resnet50_non_stem():
    import csv
    with open(os.path.join(ROOT, "datasets", "resnet50.csv"), newline="") as fh:
        rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(fh))[1:] if r]
    return sorted(s for s in set(rows) if s[2] % 64 == 0)


def test_resnet50_table_has_sixteen_non_stem_shapes():
    assert len(_resnet50_non_stem()) == 16


@pytest.mark.parametrize("shape", _resnet50_non_stem(), ids=lambda s_: "x".join(map(str, s_)))
def test_spmma_fp8_full_size_resnet50(gpu, shape):
    """b = 32, shared B, bf16 out: sampled rows against the fp64 product of the pruned operand; fused == staged."""
    import torch
    m, n, k, batch = shape
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    A = (torch.rand(batch * m * k, generator=g, device="cuda") * 4 - 2).to(torch.float8_e4m3fn)
    Bt = (torch.rand(n * k, generator=g, device="cuda") * 4 - 2).to(torch.float8_e4m3fn)
    blob = torch.empty(gpu.compress24_size(m, k, 1, batch), dtype=torch.uint8, device="cuda")
    C = torch.empty(batch * m * n, dtype=torch.bfloat16, device="cuda")
    gpu.compress24_fp8(A, m, k, k, batch, m * k, blob)
    gpu.spmma_fp8(blob, Bt, C, m, n, k, batch)
    Cf = torch.empty_like(C)
    gpu.spmma_fused_fp8(A, Bt, Cf, m, n, k, batch=batch)
    gpu.prune24_fp8(A, A, batch * m, k, k, gpu.PRUNE_STRIP)
    torch.cuda.synchronize()
    assert torch.equal(C.view(torch.int16), Cf.view(torch.int16)), f"{shape}: fused != staged"
    rng = np.random.default_rng(k)
    rows = np.unique(np.concatenate([rng.integers(0, batch * m, 64), [0, m - 1, batch * m - 1]]))
    ri = torch.from_numpy(rows).cuda()
    Ar = val64(A.view(torch.uint8).view(batch * m, k)[ri].cpu().numpy(), "e4m3")
    B = val64(bytes_of(Bt), "e4m3").reshape(n, k)
    ref, absref = Ar @ B.T, np.abs(Ar) @ np.abs(B).T
    got = C.view(batch * m, n)[ri].float().cpu().numpy().astype(np.float64)
    bound = ROUND["bf16"] * np.abs(ref) + 2.0 * k * 2.0 ** -24 * absref + TINY["bf16"]
    assert float((np.abs(got - ref) / bound).max()) <= 1.0, f"{shape}"


def test_compress_spmma_fp8_graph_capture_replays(gpu):
    import torch
    m, n, k, batch = 196, 256, 512, 4
    g = torch.Generator(device="cuda").manual_seed(5)
    A = (torch.rand(batch * m * k, generator=g, device="cuda") * 2 - 1).to(torch.float8_e5m2)
    Bt = (torch.rand(n * k, generator=g, device="cuda") * 2 - 1).to(torch.float8_e4m3fn)
    rs = torch.rand(m, generator=g, device="cuda") + 0.5
    blob = torch.empty(gpu.compress24_size(m, k, 1, batch), dtype=torch.uint8, device="cuda")
    C = torch.empty(batch * m * n, dtype=torch.float16, device="cuda")

    def step():
        gpu.compress24_fp8(A, m, k, k, batch, m * k, blob)
        gpu.spmma_fp8(blob, Bt, C, m, n, k, batch, row_scale=rs, a_dtype=A.dtype)
    step()
    torch.cuda.synchronize()
    want = C.clone()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    C.fill_(7.0)
    blob.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(C.view(torch.int16), want.view(torch.int16))


def test_spmma_fp8_driver_cli_contract(gpu):
    bins = os.path.join(ROOT, "examples", "bin")
    if not os.path.exists(os.path.join(bins, "spmma_fp8")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "-j4"], check=True, capture_output=True)

    def run(*args):
        return subprocess.run([os.path.join(bins, "spmma_fp8")] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    for argv in [(196, 64, 128, 4), (784, 256, 1152, 2), (130, 72, 192, 3)]:
        out = run(*argv)
        assert out.returncode == 0, out.stdout + out.stderr
        labels = [l.split(":")[0] for l in out.stdout.strip().splitlines()]
        assert labels[:3] == ["Pruning Time (ms)", "Compression Time (ms)", "SpMMA Time (ms)"]
        assert all(float(l.split(":")[1]) > 0.0 for l in out.stdout.strip().splitlines()[:3])
        assert "Correct: yes" in out.stdout and "Fused matches: yes" in out.stdout
    bad = run(1, 2)
    assert bad.returncode != 0 and "Usage: ./spmma_fp8 m n k b" in bad.stdout
