#!/usr/bin/env python3
"""The 1-byte 2:4 kernels against their dense denominators, per layer of a shape table (default: ResNet-50, b = 32).

For every unique (m, n, k, b) of datasets/<table>.csv with k % 64 == 0 (the stem layer, k = 147, is outside the 1-byte
kernels' constraints), one A of b matrices and one shared B ([n][k] for the 1-byte kernels).  Device times of one call in ms,
by hipGraph replay (graph_time_ms), all in one run:
  gemm_fp8    sm_gemm_rowmajor_fp8, e4m3 x e4m3, bf16 out            (dense, v_mfma_f32_16x16x128_f8f6f4)
  spmma_fp8   sm_spmma_fp8 on the compressed A, bf16 out             (2:4, v_smfmac_f32_16x16x128_fp8_fp8)
  gemm_f16    sm_gemm_rowmajor_f16, fp16 in and out                  (dense, the 16-bit denominator)
  gemm_i8     sm_gemm_rowmajor_i8, int32 out                         (dense, v_mfma_i32_16x16x64_i8)
  spmma_i8    sm_spmma_i8 on the compressed A, int32 out             (2:4, v_smfmac_i32_16x16x128_i8)
  vendor_fp8  torch._scaled_mm (unit scales, bf16 out) when this torch build runs it (--vendor; a yardstick only)
Per kernel: the share of its roofline, max(bytes / 8 TB/s, flops / peak) over the time, and which of the two bounds it
('b' bytes, 'f' flops).  bytes = each operand read once and C written once (the blob for the 2:4 kernels); flops = 2 m n k b
dense-equivalent; peak = the dense instruction rate (fp16 2.5, fp8 / int8 5 P/s) and twice that for the 2:4 kernels.
Ratios: spmma / gemm for fp8 and int8, gemm_fp8 / gemm_f16, gemm_fp8 / vendor.  Sums are weighted by the table's rows."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
PEAK = {"gemm_fp8": 5.0e15, "spmma_fp8": 10.0e15, "gemm_f16": 2.5e15, "gemm_i8": 5.0e15, "spmma_i8": 10.0e15, "vendor_fp8": 5.0e15}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="resnet50")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--vendor", action="store_true", help="add torch._scaled_mm as a vendor yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sm = ge.load_package()
    sm.device_check()
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

    kinds = ["gemm_fp8", "spmma_fp8", "gemm_f16", "gemm_i8", "spmma_i8"]
    vendor_ok = False
    if args.vendor:
        try:
            a = torch.zeros(32, 64, device=dev).to(torch.float8_e4m3fn)
            b = torch.zeros(32, 64, device=dev).to(torch.float8_e4m3fn)
            one = torch.ones((), device=dev)
            torch._scaled_mm(a, b.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16)
            torch.cuda.synchronize()
            vendor_ok = True
            kinds.append("vendor_fp8")
        except Exception as e:  # noqa: BLE001 -- reported, not hidden
            emit(f"# vendor_fp8: torch._scaled_mm does not run on this build (torch {torch.__version__}): {type(e).__name__}: "
                 + str(e).splitlines()[0][:160])
    ratios = ["fp8_sp_over_dense", "i8_sp_over_dense", "fp8_over_f16"] + (["fp8_over_vendor"] if vendor_ok else [])
    emit("m,n,k,b,cnt," + ",".join(f"{x}_ms" for x in kinds) + "," + ",".join(f"{x}_roof" for x in kinds) + "," + ",".join(ratios))
    tot = {x: 0.0 for x in kinds}
    g = torch.Generator(device=dev).manual_seed(3)
    for (m, n, k, b), cnt in uniq:
        if k % 64 != 0:
            emit(f"# {m},{n},{k},{b}: skipped (k % 64 != 0)")
            continue
        t, by = {}, {}
        fl = 2.0 * m * n * k * b
        blob8 = sm.compress24_size(m, k, 1, b)
        # fp8
        A = (torch.rand(b * m * k, generator=g, device=dev) * 2 - 1).to(torch.float8_e4m3fn)
        Bt = (torch.rand(n * k, generator=g, device=dev) * 2 - 1).to(torch.float8_e4m3fn)
        C = torch.empty(b * m * n, dtype=torch.bfloat16, device=dev)
        blob = torch.empty(blob8, dtype=torch.uint8, device=dev)
        sm.compress24_fp8(A, m, k, k, b, m * k, blob)
        t["gemm_fp8"] = sm.graph_time_ms(lambda: sm.gemm_rowmajor_fp8(A, Bt, C, m, n, k, batch=b), iters=args.iters)
        t["spmma_fp8"] = sm.graph_time_ms(lambda: sm.spmma_fp8(blob, Bt, C, m, n, k, b), iters=args.iters)
        by["gemm_fp8"] = b * m * k + n * k + 2 * b * m * n
        by["spmma_fp8"] = blob8 + n * k + 2 * b * m * n
        if vendor_ok:
            one = torch.ones((), device=dev)
            A2, B2 = A.view(b * m, k), Bt.view(n, k)
            t["vendor_fp8"] = sm.graph_time_ms(lambda: torch._scaled_mm(A2, B2.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16),
                                               iters=args.iters)
            by["vendor_fp8"] = by["gemm_fp8"]
        del A, Bt, C, blob
        # int8
        Ai = torch.randint(-128, 128, (b * m * k,), generator=g, device=dev, dtype=torch.int8)
        Bi = torch.randint(-128, 128, (n * k,), generator=g, device=dev, dtype=torch.int8)
        Ci = torch.empty(b * m * n, dtype=torch.int32, device=dev)
        blob = torch.empty(blob8, dtype=torch.uint8, device=dev)
        sm.compress24(Ai, m, k, k, b, m * k, blob)
        t["gemm_i8"] = sm.graph_time_ms(lambda: sm.gemm_rowmajor_i8(Ai, Bi, Ci, m, n, k, batch=b), iters=args.iters)
        t["spmma_i8"] = sm.graph_time_ms(lambda: sm.spmma_i8(blob, Bi, Ci, m, n, k, b), iters=args.iters)
        by["gemm_i8"] = b * m * k + n * k + 4 * b * m * n
        by["spmma_i8"] = blob8 + n * k + 4 * b * m * n
        del Ai, Bi, Ci, blob
        # fp16 dense (row-major k x n B, as sm_gemm_rowmajor_f16 takes it)
        A16 = torch.empty(b * m * k, dtype=torch.float16, device=dev)
        sm.fill_uniform(A16, 5, -1.0, 1.0)
        B16 = torch.empty(k * n, dtype=torch.float16, device=dev)
        sm.fill_uniform(B16, 6, -1.0, 1.0)
        C16 = torch.empty(b * m * n, dtype=torch.float16, device=dev)
        t["gemm_f16"] = sm.graph_time_ms(lambda: sm.gemm_rowmajor(A16, B16, C16, m, n, k, batch=b), iters=args.iters)
        by["gemm_f16"] = 2 * b * m * k + 2 * n * k + 2 * b * m * n
        del A16, B16, C16
        roof = {}
        for x in kinds:
            tot[x] += cnt * t[x]
            tb, tf = by[x] / HBM, fl / PEAK[x]
            roof[x] = "%.2f%s" % (max(tb, tf) / (t[x] * 1e-3), "b" if tb >= tf else "f")
        rv = [t["spmma_fp8"] / t["gemm_fp8"], t["spmma_i8"] / t["gemm_i8"], t["gemm_fp8"] / t["gemm_f16"]]
        if vendor_ok:
            rv.append(t["gemm_fp8"] / t["vendor_fp8"])
        emit("%d,%d,%d,%d,%d," % (m, n, k, b, cnt) + ",".join("%.4f" % t[x] for x in kinds) + "," + ",".join(roof[x] for x in kinds) + "," +
             ",".join("%.2f" % v for v in rv))
    emit("# sums (ms, weighted by table rows, stem layer excluded): " + "  ".join("%s %.3f" % (x, tot[x]) for x in kinds))
    emit("# sum spmma_fp8 / sum gemm_fp8 = %.2f   sum spmma_i8 / sum gemm_i8 = %.2f   sum gemm_fp8 / sum gemm_f16 = %.2f"
         % (tot["spmma_fp8"] / tot["gemm_fp8"], tot["spmma_i8"] / tot["gemm_i8"], tot["gemm_fp8"] / tot["gemm_f16"])
         + ("   sum gemm_fp8 / sum vendor_fp8 = %.2f" % (tot["gemm_fp8"] / tot["vendor_fp8"]) if vendor_ok else ""))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
