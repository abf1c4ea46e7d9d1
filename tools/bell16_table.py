#!/usr/bin/env python3
"""Blocked-ELL SpMM on the 16-bit matrix cores against its yardsticks, per layer of a shape table (default: ResNet-50, b = 32).

For every unique (m, n, k, b) of datasets/<table>.csv with k % 4 == 0 (the 7x7x3 stem layer has odd k and no 2 x 2 Blocked-ELL
operand, as in bin/sweep), A has 2 x 2 blocks and half of the block columns of every block row (ascending, as every producer
writes them), one A and one C per batch entry and B shared -- the operand of the reference's driver.  Times, in ms:
  bell_f16   sm_spmm_bell_batched_f16, hipGraph replay (graph_time_ms)
  bell_bf16  sm_spmm_bell_batched_bf16, the same way
  gemm_f16   sm_gemm_batched_f16 on the same m, n, k, b with a shared B (the dense fp16 product)
  bell_f32   sm_spmm_bell_batched_f32 (the dense-expansion route), HIP event pair over --reps calls: it cannot be captured
The sums are weighted by the number of table rows of each shape.  For the four shapes of bench.py's bell_stage it also prints
the roofline fraction of the f16 kernel: bytes = b (rows ell_cols 2 + ceil(rows/bs) bcols 8 + rows n 2) + cols n 2,
roof = max(bytes / 8 TB/s, 2 rows n cols b / 2.5 PF/s).  One buffer set per shape (operands may sit in the Infinity Cache for
the small layers)."""
import argparse
import csv
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
MFMA_F16 = 2.5e15
BELL_STAGE = [(784, 256, 2304, 32), (12544, 64, 576, 32), (196, 512, 4608, 32), (3136, 128, 1152, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="resnet50")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sm = ge.load_package()
    sm.device_check()
    L = sm.lib()
    dev = torch.device("cuda", 0)
    path = args.table if args.table.endswith(".csv") else os.path.join(ROOT, "datasets", args.table + ".csv")
    rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(open(path)))[1:] if r]
    uniq = []
    for r in rows:
        if r not in [u for u, _ in uniq]:
            uniq.append((r, rows.count(r)))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("m,n,k,b,cnt,bell_f16_ms,bell_bf16_ms,gemm_f16_ms,bell_f32_ms,f16_over_gemm,f32_over_f16")
    tot = dict(f16=0.0, bf16=0.0, gemm=0.0, f32=0.0)
    res = {}
    g = torch.Generator(device=dev).manual_seed(11)
    for (m, n, k, b), cnt in uniq:
        if k % 4 != 0:
            continue
        bs, ell_cols = 2, k // 2
        bcols = ell_cols // bs
        idxs = [torch.rand(m // bs, k // bs, generator=g, device=dev).argsort(dim=1)[:, :bcols].sort(dim=1).values.to(torch.int64).contiguous().view(-1)
                for _ in range(b)]
        t = {}
        for sfx, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            vals = torch.empty(b * m * ell_cols, dtype=dt, device=dev)
            sm.fill_uniform(vals, 77, -0.5, 0.5)
            B = torch.empty(k * n, dtype=dt, device=dev)
            sm.fill_uniform(B, 78, -0.5, 0.5)
            C = torch.empty(b * m * n, dtype=dt, device=dev)
            vl = [vals[i * m * ell_cols:(i + 1) * m * ell_cols] for i in range(b)]
            cl = [C[i * m * n:(i + 1) * m * n] for i in range(b)]
            t[sfx] = sm.graph_time_ms(lambda: sm.spmm_bell_batched(vl, idxs, B, cl, m, k, bs, ell_cols, n), iters=args.reps)
            if sfx == "f16":
                A = torch.empty(b * m * k, dtype=dt, device=dev)
                sm.fill_uniform(A, 79, -0.5, 0.5)
                Ap = torch.tensor([A.data_ptr() + 2 * j * m * k for j in range(b)], dtype=torch.int64, device=dev)
                Bp = torch.tensor([B.data_ptr()] * b, dtype=torch.int64, device=dev)
                Cp = torch.tensor([C.data_ptr() + 2 * j * m * n for j in range(b)], dtype=torch.int64, device=dev)
                t["gemm"] = sm.graph_time_ms(lambda: sm.gemm_batched(Ap, Bp, Cp, m, n, k, b, "f16"), iters=args.reps)
                del A
            del vals, C
        vals = torch.empty(b * m * ell_cols, dtype=torch.float32, device=dev)
        sm.fill_uniform(vals, 77, -0.5, 0.5)
        B = torch.empty(k * n, dtype=torch.float32, device=dev)
        sm.fill_uniform(B, 78, -0.5, 0.5)
        C = torch.empty(b * m * n, dtype=torch.float32, device=dev)
        nb = ctypes.c_size_t(0)
        L.sm_spmm_bell_batched_workspace_size(m, k, b, ctypes.byref(nb))
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        PA = ctypes.c_void_p * b
        pv = PA(*[vals.data_ptr() + 4 * i * m * ell_cols for i in range(b)])
        pi = PA(*[x.data_ptr() for x in idxs])
        pc = PA(*[C.data_ptr() + 4 * i * m * n for i in range(b)])

        def f32():
            rc = L.sm_spmm_bell_batched_f32(pv, pi, m, k, bs, ell_cols, B.data_ptr(), pc, n, b, 1.0, 0.0, ws.data_ptr(),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if rc != 0:
                raise RuntimeError(L.sm_last_error().decode())
        f32()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            f32()
        e1.record()
        torch.cuda.synchronize()
        t["f32"] = e0.elapsed_time(e1) / args.reps
        del vals, C, ws, idxs
        for key in tot:
            tot[key] += cnt * t[key]
        res[(m, n, k, b)] = t
        emit("%d,%d,%d,%d,%d,%.4f,%.4f,%.4f,%.4f,%.2f,%.1f" % (m, n, k, b, cnt, t["f16"], t["bf16"], t["gemm"], t["f32"],
                                                             t["f16"] / t["gemm"], t["f32"] / t["f16"]))
    emit("# sums (ms, weighted by table rows): bell_f16 %.3f  bell_bf16 %.3f  gemm_f16 %.3f  bell_f32 %.3f" %
         (tot["f16"], tot["bf16"], tot["gemm"], tot["f32"]))
    emit("# sum bell_f16 / sum gemm_f16 = %.2f (target <= 1.5); sum bell_f32 / sum bell_f16 = %.1f (target >= 4)" %
         (tot["f16"] / tot["gemm"], tot["f32"] / tot["f16"]))
    emit("# bell_stage shapes: m,n,k,b,bytes,flops,roof_us,bell_f16_us,frac (target >= 0.5),bound")
    for (m, n, k, b) in BELL_STAGE:
        bs, ell_cols = 2, k // 2
        by = b * (m * ell_cols * 2 + ((m + bs - 1) // bs) * (ell_cols // bs) * 8 + m * n * 2) + k * n * 2
        fl = 2.0 * m * n * k * b
        roof = max(by / HBM, fl / MFMA_F16)
        t = res.get((m, n, k, b))
        if t is None:
            emit("# %d,%d,%d,%d: not in the table" % (m, n, k, b))
            continue
        emit("# %d,%d,%d,%d,%d,%.3e,%.2f,%.2f,%.2f,%s" % (m, n, k, b, by, fl, roof * 1e6, t["f16"] * 1e3, roof * 1e3 / t["f16"],
                                                          "bytes" if by / HBM >= fl / MFMA_F16 else "flops"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
