"""What the GPU parity tests share: the one bound every GEMM-type comparison is held to (check_close), the session's margin list and its
report file, and the basic host / device helpers.  MARGINS and _REPORTS_WRITTEN are the session's state: there is ONE of each, here, and
every test module appends to them through this module."""
import numpy as np

FP16_TOL = 1e-2
FP32_TOL = 1e-3


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def to_dev(a):
    import torch
    return torch.from_numpy(a).cuda()


def torch_dtype(np_dtype):
    import torch
    return {np.float16: torch.float16, np.float32: torch.float32, np.float64: torch.float64}[np_dtype]


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rand(rng, n, dtype, kind="uniform"):
    if kind == "ties":
        return rng.integers(-3, 4, n).astype(dtype)
    if kind == "u01":
        return rng.uniform(0, 1, n).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


# What the arithmetic allows, not just what north_star asks: the kernels accumulate in fp32 (k products, any order)
# and round once to the output type, the oracle accumulates in fp64 and rounds once.  So
#     |got - ref| <= ROUND[out] * |ref|  +  2 * k * ACC[out] * sum_k |a*b|
# (one rounding of the result, half an ulp each side plus a possible double-rounding ulp; Higham's k*u bound on the
# fp32 accumulation with a factor 2 for alpha/beta and fused-multiply-add differences).  A dropped k-slot changes a
# result by ~|a*b| ~ scale/k, two orders of magnitude above this bound at k = 1024; the old 1e-2 * scale bound would
# have let it pass.  The looser north_star tolerance (1e-2 / 1e-3 relative) is implied and still asserted.
ROUND = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7, "f32": 2.0 ** -22, "f64": 2.0 ** -51}
ACC = {"f16": 2.0 ** -24, "bf16": 2.0 ** -24, "f32": 2.0 ** -24, "f64": 2.0 ** -53}
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -126, "f32": 2.0 ** -126, "f64": 0.0}   # one subnormal step of the output type
MARGINS = []   # (what, max err / bound) of every comparison made: written out by the modules' margin reports


def check_close(got, ref, scale, tol, what, k, out="f16"):
    got64, ref64 = got.astype(np.float64), ref.astype(np.float64)
    err = np.abs(got64 - ref64)
    scale = np.maximum(scale, 0.0)
    bad = err > tol * np.maximum(scale, 1e-30)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside north_star tol {tol}; max err {err.max():.3e}"
    bound = ROUND[out] * np.abs(ref64) + 2.0 * max(int(k), 1) * ACC[out] * scale + TINY[out]
    ratio = float((err / bound).max()) if err.size else 0.0
    MARGINS.append((what, ratio))
    assert ratio <= 1.0, (f"{what}: max err / (rounding + accumulation bound) = {ratio:.3f} > 1 "
                          f"(max err {err.max():.3e}, k = {k}, out = {out})")


_REPORTS_WRITTEN = []


def write_margin_report(lines):
    """Print a margin report and keep it in the run's output directory: the first report of a session starts the file anew, a
    later module's report follows it."""
    import os
    print("\n".join(lines))
    mode = "a" if _REPORTS_WRITTEN else "w"
    _REPORTS_WRITTEN.append(len(lines))
    try:
        d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_margins.txt"), mode) as fh:
            fh.write("\n".join(lines) + "\n")
    except OSError:
        pass


def bf16_bits(rng, n, kind="uniform"):
    """n random bfloat16 values as uint16 bit patterns (torch's CPU conversion, round to nearest even)."""
    import torch
    x = rng.integers(-3, 4, n).astype(np.float32) if kind == "ties" else rng.uniform(-1, 1, n).astype(np.float32)
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def bf16_f64(b):
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


SPLIT_TOL = {3: 2.0 ** -21, 2: 2.0 ** -13}  # sm_spmma_fused_f32_split: |error| <= SPLIT_TOL * sum |a||b| on top of the fp32 accumulation bound


def split_bound(planes, k, scale, ref):
    """The bound of both split forms against the fp64 product: the dropped piece products (SPLIT_TOL) and 2 k fp32 accumulation steps, each
    relative to scale = sum |a||b| (+ |beta||C0|), and one rounding of the result."""
    return (SPLIT_TOL[planes] + 2.0 * k * 2.0 ** -24) * scale + 2.0 ** -22 * np.abs(ref) + 1e-30


# the stream-K tests of more than one file: a workspace whose written slots show, and whether any was written
def _sk_ws(gpu):
    import torch
    ws = gpu.spmma_fused_workspace()
    ws[4096:].fill_(0xff)   # so that a written slot shows (the flags -- the first 4 KiB -- must be zero before a call)
    return ws


def _sk_ran(ws):
    return bool((ws[4096:] != 0xff).any().item())
