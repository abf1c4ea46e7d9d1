"""The bias / activation / residual epilogues of the 16-bit 2:4 matmul (sm_spmma_*_ex, sm_spmma_fused_*_ex) on the GPU:
D = act(alpha * A_2:4 . B + beta * R + bias), fp32 until the one final rounding (include/sparsifyme.h)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the project's bound for GEMM-type results (tests/parity_testlib.py): |got - ref| <= ROUND * |ref| + 2 k ACC * sum|ab| + TINY
ROUND = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
ACC = {"f16": 2.0 ** -24, "bf16": 2.0 ** -24}
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -126}

# (m, n, k, batch): every kernel family of the staged and fused dispatch (the list of test_fused_equals_staged, thinned, + the
# single-tile big form), a column tail, row tails, batch > 1
SHAPES = [(128, 64, 64, 1), (196, 512, 256, 2), (784, 256, 1024, 2), (130, 72, 192, 1), (96, 64, 128, 3), (3136, 128, 1152, 1),
          (300, 136, 320, 2), (300, 520, 128, 2), (260, 520, 576, 1), (128, 256, 128, 1), (2200, 264, 320, 4)]
SPAN = (128, 64, 147, 2)          # ragged k: the span form of the fused path
RAGGED_N = (130, 50, 128, 1)      # n % 8 != 0: the generic staged kernel's per-element store (the fused path does not take it)
IDS = lambda s_: "x".join(map(str, s_))  # noqa: E731


def _tdt(bf):
    import torch
    return torch.bfloat16 if bf else torch.float16


class Case:
    """Operands of one problem on the device: dense A (uniform(-1, 1) rounded to the type), its blob, B."""

    def __init__(self, gpu, shape, bf, shared_b=True, seed=0, nan_at=None):
        import torch
        self.gpu, self.shape, self.bf, self.tdt = gpu, shape, bf, _tdt(bf)
        m, n, k, batch = shape
        g = torch.Generator().manual_seed(0xE91 + seed + m * 3 + n + k * 5)
        A = (torch.rand(batch * m * k, generator=g) * 2 - 1).to(self.tdt)
        if nan_at is not None:
            A[nan_at] = float("nan")
        nb = 1 if shared_b else batch
        B = (torch.rand(nb * k * n, generator=g) * 2 - 1).to(self.tdt)
        self.A, self.B, self.strideB, self.gen = A, B, (0 if shared_b else k * n), g
        self.dA, self.dB = A.cuda(), B.cuda()
        self.blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
        gpu.compress24(self.dA, m, k, k, batch, m * k, self.blob)

    def rand(self, count, dtype=None):
        import torch
        return (torch.rand(count, generator=self.gen) * 2 - 1).to({None: self.tdt, "f32": torch.float32}.get(dtype, dtype))

    def run(self, path, D, alpha=1.0, beta=0.0, epilogue=None):
        m, n, k, batch = self.shape
        if path == "staged":
            self.gpu.spmma(self.blob, self.dB, D, m, n, k, batch, self.strideB, alpha=alpha, beta=beta, epilogue=epilogue)
        else:
            self.gpu.spmma_fused(self.dA, self.dB, D, m, n, k, batch=batch, strideB=self.strideB, alpha=alpha, beta=beta, epilogue=epilogue)

    def run_raw(self, path, D, alpha, beta, ep_struct):
        """The _ex entry point itself, with a NULL or a given sm_epilogue_t."""
        import torch
        m, n, k, batch = self.shape
        sfx = "bf16" if self.bf else "f16"
        L = self.gpu.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ep = ctypes.addressof(ep_struct) if ep_struct is not None else None
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        if path == "staged":
            rc = getattr(L, "sm_spmma_%s_ex" % sfx)(p(self.blob), p(self.dB), p(D), m, n, k, batch, self.strideB, m * n, alpha, beta, ep, st)
        else:
            rc = getattr(L, "sm_spmma_fused_%s_ex" % sfx)(p(self.dA), p(self.dB), p(D), m, n, k, k, batch, m * k, self.strideB, m * n, alpha,
                                                         beta, ep, st)
        assert rc == 0, (rc, L.sm_last_error())


def bits(t):
    import torch
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} elements differ, first at {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"


def paths_for(shape):
    return ["staged"] if shape[1] % 8 else ["staged", "fused"]


ALL_SHAPES = SHAPES + [SPAN, RAGGED_N]


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_plain_epilogue_is_the_plain_entry_point_and_residual_out_of_place(gpu, shape, bf):
    """(1) _ex with a NULL epilogue and with an all-default one equals the existing entry point bit for bit, beta = 0 and beta = 0.5
    with R == D; (2) R a copy of C, D a fresh buffer, beta = 0.5: D is what the existing entry point leaves in C (the vectorised
    residual path against the per-element path), and R is unchanged."""
    import torch
    m, n, k, batch = shape
    for shared_b in ([True, False] if batch > 1 and shape in (SHAPES[1], SHAPES[4], SHAPES[6]) else [True]):
        c = Case(gpu, shape, bf, shared_b)
        C0 = c.rand(batch * m * n).cuda()
        for path in paths_for(shape):
            for beta in (0.0, 0.5):
                want = C0.clone()
                c.run(path, want, alpha=0.75, beta=beta)
                got = C0.clone()
                c.run_raw(path, got, 0.75, beta, None)
                same_bits(got, want, f"{path} NULL epilogue beta={beta}")
                got = C0.clone()
                st = gpu.EpilogueStruct()
                st.R, st.strideR = got.data_ptr(), m * n
                c.run_raw(path, got, 0.75, beta, st)
                same_bits(got, want, f"{path} default epilogue beta={beta}")
                got = C0.clone()
                c.run(path, got, alpha=0.75, beta=beta, epilogue=gpu.Epilogue())
                same_bits(got, want, f"{path} Epilogue() beta={beta}")
            R = C0.clone()
            D = torch.full_like(C0, 7.0)
            c.run(path, D, alpha=0.75, beta=0.5, epilogue=gpu.Epilogue(residual=R))
            same_bits(D, want, f"{path} residual out of place")
            same_bits(R, C0, f"{path} residual operand modified")


def test_misaligned_d_and_r_take_the_per_element_store(gpu):
    """D and R that are only 2-byte aligned: the per-element fallback of the epilogue routine, against the existing entry point."""
    import torch
    shape = (130, 72, 192, 1)
    m, n, k, batch = shape
    for bf in (False, True):
        c = Case(gpu, shape, bf)
        buf0 = c.rand(m * n + 8).cuda()
        for path in ("staged", "fused"):
            want = buf0.clone()
            c.run(path, want[1:1 + m * n], alpha=0.75, beta=0.5)
            Rb = buf0.clone()
            Db = torch.full_like(buf0, 7.0)
            c.run(path, Db[1:1 + m * n], alpha=0.75, beta=0.5, epilogue=gpu.Epilogue(residual=Rb[1:1 + m * n]))
            same_bits(Db[1:1 + m * n], want[1:1 + m * n], f"{path} misaligned")
            assert float(Db[0]) == 7.0 and bool((Db[1 + m * n:] == 7.0).all())
            # an aligned D with a misaligned R falls back too
            D2 = torch.full((m * n,), 7.0, dtype=c.tdt, device="cuda")
            c.run(path, D2, alpha=0.75, beta=0.5, epilogue=gpu.Epilogue(residual=Rb[1:1 + m * n]))
            same_bits(D2, want[1:1 + m * n], f"{path} misaligned R only")


def relu_rule(x):
    """max(x, 0) as the header documents it: +0 for every x <= 0 (-0 included), NaN stays NaN."""
    import torch
    return torch.where(x > 0, x, torch.where(x != x, x, torch.zeros_like(x)))


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_relu_commutes_with_rounding(gpu, shape, bf):
    """(3) act = RELU / CLIPPED_RELU (act_arg exactly representable in the output type), no bias: D == act(C_plain) on the rounded
    output of the existing entry point, bit for bit (rounding is monotone and keeps 0 and act_arg)."""
    import torch
    m, n, k, batch = shape
    c = Case(gpu, shape, bf)
    for path in paths_for(shape):
        plain = torch.empty(batch * m * n, dtype=c.tdt, device="cuda")
        c.run(path, plain, alpha=0.5)
        assert bool((plain < 0).any()) and bool((plain > 0.5).any())
        D = torch.full_like(plain, 7.0)
        c.run(path, D, alpha=0.5, epilogue=gpu.Epilogue(act="relu"))
        same_bits(D, relu_rule(plain), f"{path} relu")
        D = torch.full_like(plain, 7.0)
        c.run(path, D, alpha=0.5, epilogue=gpu.Epilogue(act="clipped_relu", act_arg=0.5))
        same_bits(D, torch.clamp(relu_rule(plain), max=0.5), f"{path} clipped relu")


def combos(gpu, c, m, n, batch, R):
    bcol, brow = c.rand(n, "f32").cuda(), c.rand(m, "f32").cuda()
    return [("bias col + relu", 0.0, lambda D: gpu.Epilogue(bias=bcol, act="relu")),
            ("bias row + residual + hardswish", 1.0, lambda D: gpu.Epilogue(bias=brow, bias_dim="row", act="hardswish", residual=R)),
            ("residual + leaky", -0.5, lambda D: gpu.Epilogue(act="leaky_relu", act_arg=0.1, residual=R)),
            ("bias col + in-place residual + relu6", 1.0, lambda D: gpu.Epilogue(bias=bcol, act="relu6")),
            ("bias row only", 0.0, lambda D: gpu.Epilogue(bias=brow, bias_dim="row"))]


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + [SPAN], ids=IDS)
def test_fused_ex_equals_staged_ex(gpu, shape, bf):
    """(4) sm_spmma_fused_*_ex == sm_compress24 + sm_spmma_*_ex bit for bit, for every epilogue combination."""
    m, n, k, batch = shape
    for shared_b in ([True, False] if batch > 1 and shape != SPAN else [True]):
        c = Case(gpu, shape, bf, shared_b)
        R = c.rand(batch * m * n).cuda()
        D0 = (c.rand(batch * m * n) * 3).cuda()
        for name, beta, make in combos(gpu, c, m, n, batch, R):
            out = {}
            for path in ("staged", "fused"):
                D = D0.clone()
                c.run(path, D, alpha=3.0 / np.sqrt(k), beta=beta, epilogue=make(D))
                out[path] = D
            same_bits(out["fused"], out["staged"], f"{name} (shared_b={shared_b})")


# ---- (5) against fp64 -------------------------------------------------------------------------------------------------
def to64(t, bf):
    b = bits(t)
    if bf:
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return b.view(np.float16).astype(np.float64)


ACTS = {  # name -> (Epilogue kwargs, fp64 formula, Lipschitz constant, the linear pieces as masks of the pre-activation)
    "relu": (dict(act="relu"), lambda x: np.maximum(x, 0), 1.0, lambda x: [x < 0, x >= 0]),
    "relu6": (dict(act="clipped_relu", act_arg=6.0), lambda x: np.minimum(np.maximum(x, 0), 6.0), 1.0, lambda x: [x < 0, (x >= 0) & (x <= 6), x > 6]),
    "leaky": (dict(act="leaky_relu", act_arg=0.1), lambda x: np.where(x >= 0, x, 0.1 * x), 1.0, lambda x: [x < 0, x >= 0]),
    "leaky2": (dict(act="leaky_relu", act_arg=2.0), lambda x: np.where(x >= 0, x, 2.0 * x), 2.0, lambda x: [x < 0, x >= 0]),
    "hardswish": (dict(act="hardswish"), lambda x: x * np.minimum(np.maximum(x + 3, 0), 6) / 6, 1.5, lambda x: [x < -3, (x >= -3) & (x < 3), x >= 3]),
    "none": (dict(), lambda x: x, 1.0, lambda x: [np.ones_like(x, dtype=bool)]),
}


def fp64_reference(orc, c, R, bias, bias_dim, alpha, beta, rows=None):
    """(pre-activation, sum_k |a b|) in fp64 from the STRIP-pruned operand (the oracle's prune), for all rows or the sampled ones."""
    m, n, k, batch = c.shape
    pr = orc.prune24(bits(c.A), batch * m, k, k, orc.STRIP, bf16=c.bf)
    import torch
    A64 = to64(torch.from_numpy(pr.view(np.int16)), c.bf).reshape(batch * m, k)
    B64 = to64(c.B, c.bf).reshape(-1, k, n)
    R64 = to64(R, c.bf).reshape(batch * m, n)
    rows = np.arange(batch * m) if rows is None else rows
    pre = np.empty((rows.size, n))
    scale = np.empty((rows.size, n))
    for b in range(batch):
        sel = np.flatnonzero(rows // m == b)
        Bb = B64[b if B64.shape[0] > 1 else 0]
        pre[sel] = A64[rows[sel]] @ Bb
        scale[sel] = np.abs(A64[rows[sel]]) @ np.abs(Bb)
    bvec = bias.cpu().numpy().astype(np.float64)
    badd = bvec[None, :] if bias_dim == "col" else bvec[rows % m][:, None]
    x = alpha * pre + beta * R64[rows] + badd
    mag = abs(alpha) * scale + np.abs(beta * R64[rows]) + np.abs(badd)
    return x, mag


def check_against_fp64(got64, x, mag, k, out, act):
    kw, f, lip, pieces = ACTS[act]
    for i, piece in enumerate(pieces(x)):   # the condition, on the fp64 reference alone, before the device result is looked at
        assert piece.mean() >= 0.02, f"{act}: only {piece.mean():.3%} of the pre-activations fall in linear piece {i}"
    ref = f(x)
    bound = ROUND[out] * np.abs(ref) + lip * (2.0 * (k + 2) * ACC[out] * mag) + TINY[out]
    err = np.abs(got64 - ref)
    worst = np.argmax(err / bound)
    print(f"{act} {out}: worst err / bound = {err.flat[worst] / bound.flat[worst]:.3f}")
    assert (err <= bound).all(), f"{act}: {int((err > bound).sum())} outside the bound, worst {err.flat[worst]:.3e} vs {bound.flat[worst]:.3e} at {worst}"


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(130, 72, 64, 1), (130, 72, 256, 1), (196, 512, 1024, 2), (64, 8, 128, 3)], ids=IDS)
def test_against_fp64(gpu, orc, shape, bf):
    """(5) A, B, bias, R uniform(-1, 1), alpha = 12 / sqrt(k), beta = 1; reference: fp64 product of the oracle-pruned operand + the
    epilogue formula in fp64; bound: the project's, with k + 2 accumulation steps and the activation's Lipschitz constant."""
    import torch
    m, n, k, batch = shape
    out = "bf16" if bf else "f16"
    c = Case(gpu, shape, bf, shared_b=(m != 196))
    R = c.rand(batch * m * n)
    alpha = 12.0 / np.sqrt(k)
    for bias_dim in ("col", "row"):
        bias = c.rand(n if bias_dim == "col" else m, torch.float32)
        x, mag = fp64_reference(orc, c, R, bias, bias_dim, alpha, 1.0)
        for act in ACTS:
            for path in ("staged", "fused"):
                D = torch.full((batch * m * n,), 7.0, dtype=c.tdt, device="cuda")
                c.run(path, D, alpha=alpha, beta=1.0, epilogue=gpu.Epilogue(bias=bias.cuda(), bias_dim=bias_dim, residual=R.cuda(), **ACTS[act][0]))
                check_against_fp64(to64(D, bf).reshape(batch * m, n), x, mag, k, out, act)


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_both_bias_axes_index_exactly(gpu, bf):
    """(6) zero A, bias[j] = j + 1: D[i][j] == j + 1; the row form: D[i][j] == (i % m) + 1, batches stacked and per batch."""
    import torch
    for shape in [(130, 72, 192, 3), (300, 520, 128, 2), (96, 64, 128, 3), (128, 64, 147, 2), (130, 50, 128, 2)]:
        m, n, k, batch = shape
        for shared_b in (True, False):
            if shape[2] == 147 and not shared_b:
                continue
            c = Case(gpu, shape, bf, shared_b)
            c.dA.zero_()
            gpu.compress24(c.dA, m, k, k, batch, m * k, c.blob)
            bcol = torch.arange(1, n + 1, dtype=torch.float32, device="cuda")
            brow = torch.arange(1, m + 1, dtype=torch.float32, device="cuda")   # <= 300: exact in bf16 up to 256 only -> compare in the type
            want_col = bcol.to(c.tdt).repeat(batch * m)
            want_row = brow.to(c.tdt).repeat_interleave(n).repeat(batch)
            for path in paths_for(shape):
                D = torch.full((batch * m * n,), 7.0, dtype=c.tdt, device="cuda")
                c.run(path, D, epilogue=gpu.Epilogue(bias=bcol))
                same_bits(D, want_col, f"{path} column bias {shape}")
                D = torch.full((batch * m * n,), 7.0, dtype=c.tdt, device="cuda")
                c.run(path, D, epilogue=gpu.Epilogue(bias=brow, bias_dim="row"))
                same_bits(D, want_row, f"{path} row bias {shape}")


@pytest.mark.parametrize("bf", [False, True], ids=["f16", "bf16"])
def test_nan_reaches_d_through_every_activation(gpu, bf):
    """(7) a NaN in A (row 5, kept by the selection: NaN has the largest magnitude bits) makes row 5 of D NaN under every activation."""
    import torch
    shape = (130, 72, 192, 1)
    m, n, k, batch = shape
    c = Case(gpu, shape, bf, nan_at=5 * k + 17)
    bias = c.rand(n, torch.float32).cuda()
    for act in ACTS:
        for path in ("staged", "fused"):
            D = torch.full((m * n,), 7.0, dtype=c.tdt, device="cuda")
            c.run(path, D, epilogue=gpu.Epilogue(bias=bias, **ACTS[act][0]))
            D = D.reshape(m, n)
            assert bool(torch.isnan(D[5]).all()), f"{act} {path}: the NaN was lost"
            assert not bool(torch.isnan(D[:5]).any()) and not bool(torch.isnan(D[6:]).any())


@pytest.mark.parametrize("path", ["staged", "fused"])
def test_hipgraph_replay_gives_the_eager_bits(gpu, path):
    """(8) one _ex call with bias + residual + ReLU, captured and replayed twice (single stream): the eager call's bits."""
    import torch
    shape = (196, 512, 256, 2)
    m, n, k, batch = shape
    c = Case(gpu, shape, False)
    bias, R = c.rand(n, torch.float32).cuda(), c.rand(batch * m * n).cuda()
    ep = gpu.Epilogue(bias=bias, act="relu", residual=R)
    eager = torch.empty(batch * m * n, dtype=c.tdt, device="cuda")
    c.run(path, eager, beta=1.0, epilogue=ep)
    torch.cuda.synchronize()
    D = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.run(path, D, beta=1.0, epilogue=ep)
    for _ in range(2):
        D.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits(D, eager, f"{path} replay")


def test_full_size_residual_block_end(gpu, orc):
    """(9) the layer that ends a ResNet-50 residual block (datasets/resnet50.csv: 784 x 1024 x 256, b = 32, shared B) with bias +
    residual + ReLU against fp64 on sampled rows; fused == staged on all of it."""
    import torch
    shape = (784, 1024, 256, 32)
    m, n, k, batch = shape
    c = Case(gpu, shape, False)
    bias = c.rand(n, torch.float32)
    R = c.rand(batch * m * n)
    alpha = 12.0 / np.sqrt(k)
    ep = gpu.Epilogue(bias=bias.cuda(), act="relu", residual=R.cuda())
    out = {}
    for path in ("staged", "fused"):
        out[path] = torch.full((batch * m * n,), 7.0, dtype=c.tdt, device="cuda")
        c.run(path, out[path], alpha=alpha, beta=1.0, epilogue=ep)
    same_bits(out["fused"], out["staged"], "full size")
    rows = np.unique(np.concatenate([np.arange(0, batch * m, 97), [0, m - 1, m, batch * m - 1]]))
    x, mag = fp64_reference(orc, c, R, bias, "col", alpha, 1.0, rows)
    check_against_fp64(to64(out["fused"], False).reshape(batch * m, n)[rows], x, mag, k, "f16", "relu")


def test_epilogue_through_the_cpp_headers():
    """sparsifyme::spmma_fused(..., spmma_epilogue_t) and spmma_plan_t::multiply(..., spmma_epilogue_t) (include/sparsify.me/spmma.hxx)
    by value against a host fp64 evaluation: tests/cpp/epilogue_headers, fp16 and bfloat16."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "tests", "cpp"), "-f", "epilogue.mk"], check=True, capture_output=True)
    out = subprocess.run([os.path.join(root, "tests", "cpp", "bin", "epilogue_headers")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "MISMATCH" not in out.stdout and out.stdout.count(": ok") == 14 and "14 checks, 0 failed" in out.stdout
