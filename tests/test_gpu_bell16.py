"""Blocked-ELL x dense on the 16-bit matrix cores (sm_spmm_bell_*_{f16,bf16}, spmm_bell16.hip) against the CPU oracle: the
oracle runs on the 16-bit inputs converted exactly to fp32.  Tolerance as in the other parity tests: 1e-2 of sum |a||b| AND
the arithmetic bound (one rounding of the output type plus fp32 accumulation)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -126}
DTYPES = ["f16", "bf16"]
EMPTY_ID = np.uint64(0xFFFFFFFFFFFFFFFF)


def tdt(sfx):
    import torch
    return {"f16": torch.float16, "bf16": torch.bfloat16}[sfx]


def q16(x, sfx):
    """fp32 numpy array rounded to the 16-bit type, returned as (torch tensor on the device, exact fp32 numpy copy)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt(sfx))
    return t.cuda(), t.float().numpy()


def check_close(got, ref, scale, k, sfx, what):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    bad = err > 1e-2 * np.maximum(scale, 1e-30)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside 1e-2 sum|a||b|; max err {err.max():.3e}"
    bound = ROUND[sfx] * np.abs(ref) + 2.0 * max(int(k), 1) * 2.0 ** -24 * scale + TINY[sfx]
    ratio = float((err / bound).max()) if err.size else 0.0
    assert ratio <= 1.0, f"{what}: max err / arithmetic bound = {ratio:.3f} (max err {err.max():.3e})"


def make_ell(rng, rows, cols, bs, bcols=None, order="asc"):
    """values [rows][ell_cols] fp32 in (-0.5, 0.5), indices [ceil(rows/bs)][bcols] uint64, distinct block columns."""
    nbc = cols // bs
    bcols = max(1, nbc // 2) if bcols is None else bcols
    nbr = (rows + bs - 1) // bs
    ci = np.stack([rng.choice(nbc, bcols, replace=False) for _ in range(nbr)]).astype(np.uint64)
    if order == "asc":
        ci = np.sort(ci, axis=1)
    vals = rng.uniform(-0.5, 0.5, (rows, bcols * bs)).astype(np.float32)
    return vals, ci, bcols * bs


def dense_rows(vals, ci, rows_sel, cols, bs):
    """The dense rows `rows_sel` of the Blocked-ELL A (fp64)."""
    nbc = cols // bs
    bcols = ci.shape[1]
    out = np.zeros((len(rows_sel), cols), dtype=np.float64)
    for o, r in enumerate(rows_sel):
        idx = ci[r // bs]
        ok = idx < nbc
        colmat = idx[ok].astype(np.int64)[:, None] * bs + np.arange(bs)[None, :]
        out[o, colmat.reshape(-1)] = vals[r].reshape(bcols, bs)[ok].reshape(-1)
    return out


def run_single(gpu, sfx, vals_d, ci, B_d, C_d, rows, cols, bs, ell_cols, n, alpha, beta, ci_d=None):
    import torch
    if ci_d is None:
        ci_d = torch.from_numpy(ci.reshape(-1).view(np.int64)).cuda()
    gpu.spmm_bell(vals_d, ci_d, B_d, C_d, rows, cols, bs, ell_cols, n, alpha, beta)
    torch.cuda.synchronize()
    return C_d


def oracle(orc, vals32, ci, B32, C32, rows, cols, bs, ell_cols, n, alpha, beta):
    Cref = C32.copy().reshape(-1)
    orc.spmm_bell(np.ascontiguousarray(vals32).reshape(-1), np.ascontiguousarray(ci).reshape(-1), rows, cols, bs, ell_cols,
                  np.ascontiguousarray(B32).reshape(-1), Cref, n, alpha, beta)
    return Cref


def scale_of(vals32, ci, B32, C32, rows, cols, bs, n, alpha, beta):
    A = dense_rows(vals32, ci, range(rows), cols, bs)
    Bm = B32.reshape(n, cols).astype(np.float64)  # column-major cols x n: row j of this view is column j
    s = np.abs(alpha) * (np.abs(A) @ np.abs(Bm).T)  # rows x n
    s = s + np.abs(beta) * np.abs(C32.reshape(n, rows).T.astype(np.float64))
    return s.T.reshape(-1)  # column-major


def one_case(gpu, orc, sfx, rng, rows, cols, bs, n, alpha, beta, order="asc", ci=None, vals=None, ell_cols=None, what=""):
    if ci is None:
        vals, ci, ell_cols = make_ell(rng, rows, cols, bs, order=order)
    vals_d, vals32 = q16(vals, sfx)
    B_d, B32 = q16(rng.uniform(-0.5, 0.5, cols * n), sfx)
    C_d, C32 = q16(rng.uniform(-1, 1, rows * n), sfx)
    got = run_single(gpu, sfx, vals_d.reshape(-1), ci, B_d, C_d, rows, cols, bs, ell_cols, n, alpha, beta)
    ref = oracle(orc, vals32, ci, B32, C32, rows, cols, bs, ell_cols, n, alpha, beta)
    check_close(got.float().cpu().numpy(), ref, scale_of(vals32, ci, B32, C32, rows, cols, bs, n, alpha, beta), cols, sfx,
                what or f"{sfx} {rows}x{cols} bs {bs} n {n}")
    return got


# (block_size, rows, cols, n, (alpha, beta)): rows not a multiple of bs nor of the 128-row tile, cols not a multiple of 64
# (and not of bs for bs = 3 and 32)
SHAPES = [(1, 200, 100, 37, (1.0, 0.0)), (2, 131, 96, 5, (1.5, 0.5)), (3, 130, 200, 70, (0.75, -2.0)), (4, 257, 136, 256, (1.0, 0.0)),
          (8, 300, 264, 1, (1.5, 0.5)), (16, 140, 320, 70, (0.75, -2.0)), (32, 161, 330, 37, (1.0, 0.0)), (2, 390, 1000, 256, (0.75, -2.0)),
          (3, 77, 50, 5, (1.0, 0.0)), (2, 64, 64, 1, (1.5, 0.5))]


@pytest.mark.parametrize("sfx", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"bs{s[0]}-{s[1]}x{s[2]}-n{s[3]}" for s in SHAPES])
def test_shapes_vs_oracle(gpu, orc, sfx, shape):
    bs, rows, cols, n, (alpha, beta) = shape
    one_case(gpu, orc, sfx, np.random.default_rng(rows * 7 + cols + bs), rows, cols, bs, n, alpha, beta)


@pytest.mark.parametrize("sfx", DTYPES)
def test_beta_zero_does_not_read_c(gpu, orc, sfx):
    import torch
    rng = np.random.default_rng(3)
    rows, cols, bs, n = 150, 200, 2, 70
    vals, ci, ell_cols = make_ell(rng, rows, cols, bs)
    vals_d, vals32 = q16(vals, sfx)
    B_d, B32 = q16(rng.uniform(-0.5, 0.5, cols * n), sfx)
    C_d = torch.full((rows * n,), float("nan"), dtype=tdt(sfx), device="cuda")
    got = run_single(gpu, sfx, vals_d.reshape(-1), ci, B_d, C_d, rows, cols, bs, ell_cols, n, 1.0, 0.0)
    zeros = np.zeros(rows * n, dtype=np.float32)
    ref = oracle(orc, vals32, ci, B32, zeros, rows, cols, bs, ell_cols, n, 1.0, 0.0)
    check_close(got.float().cpu().numpy(), ref, scale_of(vals32, ci, B32, zeros, rows, cols, bs, n, 1.0, 0.0), cols, sfx, "beta 0 over NaN")


@pytest.mark.parametrize("sfx", DTYPES)
@pytest.mark.parametrize("where", ["end", "middle"])
def test_empty_blocks_are_skipped(gpu, orc, sfx, where):
    rng = np.random.default_rng(5 if where == "end" else 6)
    rows, cols, bs, n = 260, 192, 2, 37
    nbc = cols // bs
    vals, ci, ell_cols = make_ell(rng, rows, cols, bs, bcols=40)
    for br in range(ci.shape[0]):
        if where == "end":  # ascending stored blocks followed by empty ids (the fast path)
            ci[br, -3] = nbc
            ci[br, -2] = EMPTY_ID
            ci[br, -1] = nbc + 5
        else:  # empty ids between stored blocks
            ci[br, 5] = EMPTY_ID
            ci[br, 17] = nbc
    ci[7, :] = EMPTY_ID  # one block row with nothing stored
    one_case(gpu, orc, sfx, rng, rows, cols, bs, n, 1.5, 0.5, ci=ci, vals=vals, ell_cols=ell_cols, what=f"{sfx} empty ids ({where})")


@pytest.mark.parametrize("sfx", DTYPES)
@pytest.mark.parametrize("bs", [1, 2, 3, 8])
def test_block_order_does_not_change_c(gpu, orc, sfx, bs):
    """Permuting a block row's blocks together with their values gives the same C bit for bit (the generic path for the
    shuffled tiles, the fast path for the ascending ones)."""
    import torch
    rng = np.random.default_rng(40 + bs)
    rows, cols, n = 300, 700, 70
    vals, ci, ell_cols = make_ell(rng, rows, cols, bs)
    bcols = ci.shape[1]
    ci_s, vals_s = ci.copy(), vals.copy()
    for br in range(ci.shape[0]):
        perm = rng.permutation(bcols)
        ci_s[br] = ci[br, perm]
        r0, r1 = br * bs, min(rows, (br + 1) * bs)
        vals_s[r0:r1] = vals[r0:r1].reshape(r1 - r0, bcols, bs)[:, perm, :].reshape(r1 - r0, -1)
    B_d, _ = q16(rng.uniform(-0.5, 0.5, cols * n), sfx)
    C0 = rng.uniform(-1, 1, rows * n)
    outs = []
    for v, c in ((vals, ci), (vals_s, ci_s)):
        vd, _ = q16(v, sfx)
        Cd, _ = q16(C0, sfx)
        outs.append(run_single(gpu, sfx, vd.reshape(-1), c, B_d, Cd, rows, cols, bs, ell_cols, n, 0.75, -2.0))
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    one_case(gpu, orc, sfx, rng, rows, cols, bs, n, 0.75, -2.0, ci=ci_s, vals=vals_s, ell_cols=ell_cols, what=f"{sfx} shuffled bs {bs}")


@pytest.mark.parametrize("sfx", DTYPES)
def test_batched_equals_single_calls(gpu, orc, sfx):
    import torch
    rng = np.random.default_rng(21)
    rows, cols, bs, n, batch = 136, 160, 2, 70, 5
    B_d, B32 = q16(rng.uniform(-0.5, 0.5, cols * n), sfx)
    As, refs, C0s = [], [], []
    for _ in range(batch):
        vals, ci, ell_cols = make_ell(rng, rows, cols, bs)
        vd, v32 = q16(vals, sfx)
        As.append((vd.reshape(-1), torch.from_numpy(ci.reshape(-1).view(np.int64)).cuda(), v32, ci))
        C0s.append(rng.uniform(-1, 1, rows * n))
    singles = []
    for (vd, cd, _, _), c0 in zip(As, C0s):
        Cd, _ = q16(c0, sfx)
        gpu.spmm_bell(vd, cd, B_d, Cd, rows, cols, bs, ell_cols, n, 0.75, -2.0)
        singles.append(Cd)
    Cs = [q16(c0, sfx)[0] for c0 in C0s]
    Arr = ctypes.c_void_p * batch
    pv = Arr(*[a[0].data_ptr() for a in As])
    pi = Arr(*[a[1].data_ptr() for a in As])
    pc = Arr(*[c.data_ptr() for c in Cs])
    fn = getattr(gpu.lib(), "sm_spmm_bell_batched_" + sfx)
    rc = fn(pv, pi, rows, cols, bs, ell_cols, B_d.data_ptr(), pc, n, batch, 0.75, -2.0,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    del pv, pi, pc  # the host tables may go as soon as the call returns
    torch.cuda.synchronize()
    for b in range(batch):
        assert torch.equal(Cs[b].view(torch.int16), singles[b].view(torch.int16)), f"batch {b}"
        _, C32 = q16(C0s[b], sfx)
        ref = oracle(orc, As[b][2], As[b][3], B32, C32, rows, cols, bs, ell_cols, n, 0.75, -2.0)
        check_close(Cs[b].float().cpu().numpy(), ref, scale_of(As[b][2], As[b][3], B32, C32, rows, cols, bs, n, 0.75, -2.0), cols, sfx,
                    f"batched {b}")
    # the Python wrapper: the same call
    Cw = [q16(c0, sfx)[0] for c0 in C0s]
    gpu.spmm_bell_batched([a[0] for a in As], [a[1] for a in As], B_d, Cw, rows, cols, bs, ell_cols, n, 0.75, -2.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(Cw, Cs))


@pytest.mark.parametrize("sfx", DTYPES)
def test_more_than_one_launch_of_batches(gpu, sfx):
    """b = 70 runs as more than one launch (64 pointer-table entries per launch): each C equals its single-matrix call bit for bit."""
    import torch
    rng = np.random.default_rng(70)
    rows, cols, bs, n, batch = 40, 96, 2, 24, 70
    B_d, _ = q16(rng.uniform(-0.5, 0.5, cols * n), sfx)
    vl, il, singles, Cs = [], [], [], []
    for _ in range(batch):
        vals, ci, ell_cols = make_ell(rng, rows, cols, bs)
        vl.append(q16(vals, sfx)[0].reshape(-1))
        il.append(torch.from_numpy(ci.reshape(-1).view(np.int64)).cuda())
        c0 = rng.uniform(-1, 1, rows * n)
        singles.append(q16(c0, sfx)[0])
        Cs.append(q16(c0, sfx)[0])
        gpu.spmm_bell(vl[-1], il[-1], B_d, singles[-1], rows, cols, bs, ell_cols, n, 1.5, 0.5)
    gpu.spmm_bell_batched(vl, il, B_d, Cs, rows, cols, bs, ell_cols, n, 1.5, 0.5)
    torch.cuda.synchronize()
    for b in range(batch):
        assert torch.equal(Cs[b].view(torch.int16), singles[b].view(torch.int16)), f"batch {b}"


@pytest.mark.parametrize("sfx", DTYPES)
def test_stage_table_too_large_for_lds(gpu, orc, sfx):
    """cols = 30 000 with block_size 1: the per-tile stage table does not fit in LDS, every tile takes the generic path."""
    rng = np.random.default_rng(9)
    rows, cols, bs, n = 130, 30000, 1, 5
    vals, ci, ell_cols = make_ell(rng, rows, cols, bs, bcols=64)
    one_case(gpu, orc, sfx, rng, rows, cols, bs, n, 1.0, 0.0, ci=ci, vals=vals, ell_cols=ell_cols, what=f"{sfx} table over LDS")


def test_unsupported_dtype_raises_the_package_error(gpu):
    import torch
    x = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmm_bell(x, x, x, x, 2, 2, 1, 2, 2)
    with pytest.raises(gpu.SparsifymeError):
        gpu.spmm_bell_batched([x], [x], x, [x], 2, 2, 1, 2, 2)


def test_graph_capture_replays_the_eager_result(gpu):
    import torch
    rng = np.random.default_rng(31)
    rows, cols, bs, n, batch = 300, 576, 2, 64, 3
    B_d, _ = q16(rng.uniform(-0.5, 0.5, cols * n), "f16")
    vals_l, idx_l = [], []
    for _ in range(batch):
        vals, ci, ell_cols = make_ell(rng, rows, cols, bs)
        vals_l.append(q16(vals, "f16")[0].reshape(-1))
        idx_l.append(torch.from_numpy(ci.reshape(-1).view(np.int64)).cuda())
    eager = [torch.zeros(rows * n, dtype=torch.float16, device="cuda") for _ in range(batch)]
    gpu.spmm_bell_batched(vals_l, idx_l, B_d, eager, rows, cols, bs, ell_cols, n)
    torch.cuda.synchronize()
    Cs = [torch.zeros(rows * n, dtype=torch.float16, device="cuda") for _ in range(batch)]
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gpu.spmm_bell_batched(vals_l, idx_l, B_d, Cs, rows, cols, bs, ell_cols, n)
    for c in Cs:
        c.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(Cs, eager):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_f32_dispatch_of_the_wrappers(gpu, orc):
    import torch
    rng = np.random.default_rng(8)
    rows, cols, bs, n = 100, 96, 2, 37
    vals, ci, ell_cols = make_ell(rng, rows, cols, bs)
    B = rng.uniform(-1, 1, cols * n).astype(np.float32)
    C0 = rng.uniform(-1, 1, rows * n).astype(np.float32)
    ref = oracle(orc, vals, ci, B, C0, rows, cols, bs, ell_cols, n, 1.5, 0.5)
    Cd = torch.from_numpy(C0.copy()).cuda()
    gpu.spmm_bell(torch.from_numpy(vals.reshape(-1)).cuda(), torch.from_numpy(ci.reshape(-1).view(np.int64)).cuda(),
                  torch.from_numpy(B).cuda(), Cd, rows, cols, bs, ell_cols, n, 1.5, 0.5)
    torch.cuda.synchronize()
    assert np.allclose(Cd.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    Cl = [torch.from_numpy(C0.copy()).cuda() for _ in range(2)]
    gpu.spmm_bell_batched([torch.from_numpy(vals.reshape(-1)).cuda()] * 2, [torch.from_numpy(ci.reshape(-1).view(np.int64)).cuda()] * 2,
                          torch.from_numpy(B).cuda(), Cl, rows, cols, bs, ell_cols, n, 1.5, 0.5)
    torch.cuda.synchronize()
    for c in Cl:
        assert np.allclose(c.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)


BELL_STAGE = [(784, 256, 2304), (12544, 64, 576), (196, 512, 4608), (3136, 128, 1152)]


@pytest.mark.parametrize("sfx", DTYPES)
@pytest.mark.parametrize("shape", BELL_STAGE, ids=[f"{m}x{n}x{k}" for m, n, k in BELL_STAGE])
def test_full_size_bell_stage_shapes(gpu, sfx, shape):
    """The four bench shapes at b = 32 (2 x 2 blocks, half the block columns), 64 sampled rows of every batch against fp64 on the host."""
    import torch
    m, n, k = shape
    b, bs = 32, 2
    ell_cols, bcols = k // 2, k // 4
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(m + n + k)
    vals, idxs = [], []
    for _ in range(b):
        idxs.append(torch.rand(m // bs, k // bs, generator=g, device=dev).argsort(dim=1)[:, :bcols].sort(dim=1).values.to(torch.int64).contiguous())
        vals.append((torch.rand(m, ell_cols, generator=g, device=dev) - 0.5).to(tdt(sfx)))
    B = (torch.rand(n, k, generator=g, device=dev) - 0.5).to(tdt(sfx))  # column-major k x n
    Cs = [torch.empty(n, m, dtype=tdt(sfx), device=dev) for _ in range(b)]
    gpu.spmm_bell_batched([v.view(-1) for v in vals], [i.view(-1) for i in idxs], B.view(-1), [c.view(-1) for c in Cs], m, k, bs, ell_cols, n)
    torch.cuda.synchronize()
    rng = np.random.default_rng(m)
    B64 = B.float().cpu().numpy().astype(np.float64)  # [n][k]
    for bi in range(b):
        sel = np.sort(rng.choice(m, 64, replace=False))
        v32 = vals[bi][torch.from_numpy(sel).to(dev)].float().cpu().numpy()
        ci = idxs[bi].cpu().numpy().view(np.uint64)
        # dense rows of the sample: re-index values to the sampled rows
        A = np.zeros((64, k))
        for o, r in enumerate(sel):
            cols_ = (ci[r // bs].astype(np.int64)[:, None] * bs + np.arange(bs)[None, :]).reshape(-1)
            A[o, cols_] = v32[o]
        ref = A @ B64.T  # 64 x n
        scale = np.abs(A) @ np.abs(B64).T
        got = Cs[bi][:, torch.from_numpy(sel).to(dev)].float().cpu().numpy().T  # C column-major: C[j][r]
        check_close(got, ref, scale, k, sfx, f"{sfx} {m}x{n}x{k} batch {bi}")


def test_spmm_f16_driver():
    exe = os.path.join(ROOT, "examples", "bin", "spmm_f16")
    assert os.path.exists(exe), "build() makes examples/bin/spmm_f16"
    for args in (["64", "32", "64", "2"], ["784", "256", "2304", "4", "bf16"]):
        res = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        assert float(res.stdout.strip().splitlines()[-1]) > 0.0


def test_batched_spmm_half_through_the_cpp_headers(tmp_path):
    exe = tmp_path / "bell16_cpp"
    lib = os.path.join(ROOT, "sparsify.me_amd")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tests", "cpp", "bell16_cpp.cpp"), "-o", str(exe), "-L" + lib, "-lsparsifyme",
                          "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "OK" in run.stdout, run.stdout + run.stderr
